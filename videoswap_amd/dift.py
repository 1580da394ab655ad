"""DIFT semantic-point embeddings on the libvsx kernels (extract_semantic_point.py:114-205, videoswap/utils/dift_util.py).

A TAP file (`formats.load_tap`) holds, next to the point tracks, one 1280-wide DIFT feature per semantic point.  The
reference computes it with diffusers' SD pipeline in fp32 on CUDA; here:

* `SDFeaturizer` runs the SD-1.5 VAE encoder and the 2-D UNet truncated after up block `up_ft_index`
  (`AnimateDiffUNet3DModel.forward_features`) on the HIP kernels.  Each frame is encoded ONCE and its E ensemble members
  are E posterior samples of its moments (the reference encodes E identical copies: the same distribution), and
  E x `frames_per_call` images go through one UNet call with the prompt passed once.
* The ensemble mean, the bilinear upsampling to image size and the cosine similarities are
  `ops.dift_sample_points` / `ops.dift_cosine_map` (csrc/dift.hip): the upsampled [C, H, W] map the reference builds
  per query (1.76 GB of fp32 at 448x768) never exists.
* `extract_point_embedding` is the bookkeeping of extract_semantic_point.py:125-205, one kernel launch per batch of
  frames for all of its points.  Deviations: a coordinate past the image raises ValueError
  (the reference: IndexError); the object branch reads the keyframe's points once before its loop (the reference reads
  a view that its own loop overwrites, so its result depends on directory order).

Point tracks themselves (CoTracker / OpenPose propagation, extract_semantic_point.py:34-111) are an input.
"""
import os

import numpy as np
import torch

from . import ops

PROMPT_TEMPLATE = 'photo of a {}'


# ------------------------------------------------------------------------------------------------
# frames
# ------------------------------------------------------------------------------------------------
def list_frames(frame_dir):
    """[(int(stem), path)] of the .jpg / .png files of `frame_dir`, in sorted path order (extract_semantic_point.py:132)."""
    out = []
    for name in sorted(os.listdir(frame_dir)):
        stem, ext = os.path.splitext(name)
        if ext.lower() in ('.jpg', '.jpeg', '.png'):
            try:
                out.append((int(stem), os.path.join(frame_dir, name)))
            except ValueError:
                raise ValueError(f'{frame_dir}/{name}: frame files are named by their integer index') from None
    if not out:
        raise ValueError(f'{frame_dir}: no .jpg / .png frames')
    return out


def image_tensor(image):
    """PIL image or path -> [3, H, W] fp32 in [-1, 1]: `(PILToTensor()(image) / 255.0 - 0.5) * 2`
    (extract_semantic_point.py:120), at native size."""
    from PIL import Image
    if not isinstance(image, Image.Image):
        image = Image.open(image).convert('RGB')
    arr = torch.from_numpy(np.array(image.convert('RGB'), dtype=np.uint8, copy=True))
    return (arr.permute(2, 0, 1) / 255.0 - 0.5) * 2


def _wrap(v, n, what):
    """Python indexing of the reference (`map[:, y, x]`): -n <= v < 0 reads from the far edge; outside [-n, n) raises."""
    if v >= n or v < -n:
        raise ValueError(f'{what} {v} lies outside an image side of {n} pixels')
    return v + n if v < 0 else v


# ------------------------------------------------------------------------------------------------
# featurizer
# ------------------------------------------------------------------------------------------------
class SDFeaturizer:
    """dift_util.py:185-227 on the HIP kernels.  `sd_id`: one SD folder with unet/ (loaded as the 2-D UNet, no motion
    modules), vae/ (encoder only), text_encoder/ + tokenizer/ and scheduler/.  `SDFeaturizer.from_components` builds one
    from models already in memory (tests, tools/dift_bench.py)."""

    def __init__(self, sd_id='pretrained_models/stable-diffusion-v1-4', device='cuda', frames_per_call=4):
        from .clip import CLIPTextModel, load_tokenizer
        from .compat import DDIMScheduler
        from .unet import AnimateDiffUNet3DModel
        from .vae import AutoencoderKL
        unet = AnimateDiffUNet3DModel.from_pretrained_2d(sd_id, subfolder='unet',
                                                         unet_additional_kwargs={'use_motion_module': False})
        vae = AutoencoderKL.from_pretrained(sd_id, subfolder='vae')
        text_encoder = CLIPTextModel.from_pretrained(sd_id, subfolder='text_encoder')
        self._init(unet, vae, text_encoder, load_tokenizer(sd_id), DDIMScheduler.from_pretrained(sd_id, subfolder='scheduler'),
                   device, frames_per_call)

    @classmethod
    def from_components(cls, unet, vae, scheduler, text_encoder=None, tokenizer=None, device='cuda', frames_per_call=4):
        self = cls.__new__(cls)
        self._init(unet, vae, text_encoder, tokenizer, scheduler, device, frames_per_call)
        return self

    def _init(self, unet, vae, text_encoder, tokenizer, scheduler, device, frames_per_call):
        self.device = torch.device(device)
        vae.decoder = None                                   # onestep_pipe.vae.decoder = None (dift_util.py:191)
        self.unet = unet.to(device=self.device, dtype=torch.float16).eval()
        self.vae = vae.to(device=self.device, dtype=torch.float16).eval()
        self.text_encoder = None if text_encoder is None else text_encoder.to(device=self.device, dtype=torch.float16).eval()
        self.tokenizer = tokenizer
        self.scheduler = scheduler
        self.frames_per_call = int(frames_per_call)
        self.scaling_factor = float(getattr(vae.config, 'scaling_factor', 0.18215)) if hasattr(vae, 'config') else 0.18215
        self._prompts = {}
        self.timings = None                                  # tools/dift_bench.py: {'vae': s, 'unet': s} when a dict

    @torch.no_grad()
    def encode_prompt(self, prompt):
        """[1, 77, D] fp16 (StableDiffusionPipeline._encode_prompt without guidance), cached per prompt."""
        hit = self._prompts.get(prompt)
        if hit is None:
            if self.text_encoder is None or self.tokenizer is None:
                raise ValueError('SDFeaturizer: no text encoder / tokenizer: pass prompt_embeds')
            ids = self.tokenizer(prompt, padding='max_length', max_length=self.tokenizer.model_max_length,
                                 truncation=True, return_tensors='pt').input_ids
            hit = self.text_encoder(ids.to(self.device))[0].to(torch.float16)
            self._prompts[prompt] = hit
        return hit

    def _timed(self, key, fn):
        if self.timings is None:
            return fn()
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        out = fn()
        ev[1].record()
        ev[1].synchronize()
        self.timings[key] = self.timings.get(key, 0.0) + ev[0].elapsed_time(ev[1]) / 1e3
        return out

    @torch.no_grad()
    def features(self, images, prompt=None, t=261, up_ft_index=1, ensemble_size=8, generator=None, prompt_embeds=None,
                 noise=None, frames_per_call=None):
        """images [N, 3, H, W] in [-1, 1] (H, W multiples of 64) -> the UNet tap fp16 [N, E, H/16, W/16, C]
        (channels-last, the E ensemble members of a frame adjacent) for ops.dift_sample_points / dift_cosine_map.

        noise: None (drawn from `generator`) or (posterior, diffusion), each [N, E, 4, H/8, W/8]: the standard-normal
        draws of the VAE posterior sample and of `scheduler.add_noise` (dift_util.py:174-177)."""
        if images.dim() != 4 or images.shape[1] != 3:
            raise ValueError(f'images must be [N, 3, H, W], got {tuple(images.shape)}')
        N, _, H, W = images.shape
        if H % 64 or W % 64:
            raise ValueError(f'image sides must be multiples of 64 (latents multiples of 8: the UNet has no forced '
                             f'upsample size); got {H}x{W}')
        E = int(ensemble_size)
        if prompt_embeds is None:
            prompt_embeds = self.encode_prompt(prompt)
        text = prompt_embeds.to(device=self.device, dtype=torch.float16)
        if text.dim() == 2:
            text = text[None]
        if text.shape[0] != 1:
            raise ValueError('features: pass ONE prompt embedding [1, 77, D] (the cross-attention shares it across images)')
        text = text.contiguous()
        fpc = max(1, int(frames_per_call or self.frames_per_call))
        h, w = H // 8, W // 8
        timesteps = torch.tensor([int(t)], dtype=torch.long)
        out = None
        for s in range(0, N, fpc):
            n = min(fpc, N - s)
            x = images[s:s + n].to(device=self.device, dtype=torch.float16)
            moments = self._timed('vae', lambda: self.vae.encode(x).latent_dist.parameters).float()   # [n, 8, h, w]
            mean, logvar = torch.chunk(moments, 2, dim=1)
            std = torch.exp(0.5 * torch.clamp(logvar, -30.0, 20.0))
            if noise is None:
                dev = generator.device if generator is not None else self.device
                eps_p = torch.randn((n, E, 4, h, w), generator=generator, device=dev).to(self.device)
                eps_d = torch.randn((n, E, 4, h, w), generator=generator, device=dev).to(self.device)
            else:
                eps_p = noise[0][s:s + n].to(device=self.device, dtype=torch.float32)
                eps_d = noise[1][s:s + n].to(device=self.device, dtype=torch.float32)
            z = (mean[:, None] + std[:, None] * eps_p) * self.scaling_factor                      # [n, E, 4, h, w]
            z = self.scheduler.add_noise(z.reshape(n * E, 4, h, w), eps_d.reshape(n * E, 4, h, w), timesteps)
            sample = z.to(torch.float16)[:, :, None].contiguous()                                 # [n E, 4, 1, h, w]
            ft = self._timed('unet', lambda: self.unet.forward_features(sample, int(t), text, [up_ft_index]))[up_ft_index]
            if out is None:
                out = torch.empty((N, E) + tuple(ft.shape[1:]), dtype=torch.float16, device=self.device)
            out[s:s + n] = ft.view((n, E) + tuple(ft.shape[1:]))
        return out

    @torch.no_grad()
    def forward(self, img_tensor, prompt, t=261, up_ft_index=1, ensemble_size=8, generator=None, prompt_embeds=None,
                noise=None):
        """dift_util.py:198-227: img_tensor [1, 3, H, W] or [3, H, W] -> the ensemble-mean map [1, C, h, w] (fp32).
        The channels-last ensemble it came from rides along as `.vsx_ensemble` ([1, E, h, w, C] fp16), which DIFTDemo
        reads instead of the mean.  noise: None or (posterior, diffusion), each [E, 4, H/8, W/8]."""
        if img_tensor.dim() == 3:
            img_tensor = img_tensor[None]
        if noise is not None:
            noise = (noise[0][None], noise[1][None])
        ens = self.features(img_tensor, prompt, t, up_ft_index, ensemble_size, generator, prompt_embeds, noise, 1)
        mean = ens[0].float().mean(0).permute(2, 0, 1)[None]
        mean.vsx_ensemble = ens
        return mean


def _ensemble(dift):
    """[1, C, h, w] from SDFeaturizer.forward (its ensemble when it carries one) or the tap [N, E, h, w, C] itself."""
    ens = getattr(dift, 'vsx_ensemble', None)
    if ens is not None:
        return ens
    if dift.dim() == 5:
        return dift
    if dift.dim() == 4 and dift.shape[0] == 1:
        return dift.permute(0, 2, 3, 1)[:, None].to(torch.float16).contiguous()
    raise ValueError(f'expected a DIFT map [1, C, h, w] or [N, E, h, w, C], got {tuple(dift.shape)}')


def _coords(xy, device):
    return torch.tensor(np.asarray(xy, dtype=np.int32).reshape(-1, 2), device=device)[None].contiguous()


def heatmap_image(target_img, cos_map, max_yx, target_xy=None, radius=3):
    """dift_util.py:252-264: min-max normalised cosine map through matplotlib's viridis, blended 1:1 with the image,
    green dots at the best match and at the tracked point."""
    from matplotlib import colormaps
    from PIL import Image, ImageDraw
    hm = np.asarray(cos_map, dtype=np.float32)
    span = float(hm.max() - hm.min())
    hm = (hm - hm.min()) / (span if span > 0 else 1.0)
    color = (colormaps['viridis'](hm) * 255)[..., :3].astype(np.uint8)
    blended = Image.blend(target_img.convert('RGB'), Image.fromarray(color), alpha=0.5)
    draw = ImageDraw.Draw(blended)
    pts = [(int(max_yx[1]), int(max_yx[0]))] + ([tuple(int(v) for v in target_xy)] if target_xy is not None else [])
    for x, y in pts:
        draw.ellipse((x - radius, y - radius, x + radius, y + radius), fill=(0, 255, 0))
    return blended


class DIFTDemo:
    """dift_util.py:230-267 on kernels (a) / (b): same constructor and `query` arguments and return values."""

    def __init__(self, source_img, source_dift, source_img_size):
        self.source_img = source_img
        self.source_dift = source_dift
        self.source_img_size = source_img_size          # [height, width]
        self._src = _ensemble(source_dift)

    @torch.no_grad()
    def query(self, target_img, target_dift, target_img_size, query_point, target_point, visualize=False):
        """query_point / target_point: [y, x].  -> (dift_feat [C] fp32, confidence np.float32, blended PIL image or None)"""
        Hs, Ws = (int(v) for v in self.source_img_size)
        Ht, Wt = (int(v) for v in target_img_size)
        sx = _wrap(int(np.round(query_point[1])), Ws, 'query x')
        sy = _wrap(int(np.round(query_point[0])), Hs, 'query y')
        tx = _wrap(int(np.round(target_point[1])), Wt, 'target x')
        ty = _wrap(int(np.round(target_point[0])), Ht, 'target y')
        src = self._src
        src_vec, _ = ops.dift_sample_points(src, (Hs, Ws), _coords([sx, sy], src.device))
        tgt = _ensemble(target_dift)
        q = src_vec[0].contiguous()                                          # [1, C]
        vec, cos = ops.dift_sample_points(tgt, (Ht, Wt), _coords([tx, ty], tgt.device), query=q, want_cos=True)
        blended = None
        if visualize:
            cmap, yx, _ = ops.dift_cosine_map(tgt, (Ht, Wt), q)
            blended = heatmap_image(target_img, cmap[0, 0].cpu().numpy(), yx[0, 0].tolist(), (tx, ty))
        return vec[0, 0], np.float32(cos[0, 0].item()), blended


# ------------------------------------------------------------------------------------------------
# extraction (extract_semantic_point.py:125-205)
# ------------------------------------------------------------------------------------------------
def _round_tracks(tracks):
    """np.round (half to even) of pixel coordinates, as int64 (torch.round rounds half to even as well)"""
    return torch.round(tracks.float()).to(torch.int64)


def _load_batch(paths):
    imgs = [image_tensor(p) for p in paths]
    sizes = {tuple(i.shape[1:]) for i in imgs}
    if len(sizes) != 1:
        raise ValueError(f'frames of one batch differ in size: {sorted(sizes)}')
    return torch.stack(imgs)


@torch.no_grad()
def extract_point_embedding(tap_dict, frame_dir, keyframe_id, featurizer, subject_category, is_human, t=261,
                            up_ft_index=1, ensemble_size=8, frames_per_call=None, generator=None, prompt_embeds=None,
                            noise=None, confidence_threshold=0.35, vis_dir=None):
    """extract_semantic_point.py:125-205.  tap_dict: {'pred_tracks' [F, P, 2] (pixel x, y), 'point_name2id'}; frames:
    the .jpg / .png files of `frame_dir` named by frame index.  -> tap_dict with 'point_embedding' [P, C] fp32 (CPU)
    and, in the object branch, the filtered 'pred_tracks' (a new tensor; the input is not modified).

    noise: None, or {frame index: (posterior, diffusion)} with [E, 4, H/8, W/8] each (SDFeaturizer.features).
    vis_dir (object branch): writes the cosine heat map of every keyframe point over the keyframe (kernel (b))."""
    frames = list_frames(frame_dir)
    tracks = tap_dict['pred_tracks'].detach().to('cpu', torch.float32).clone()
    F_total, P = tracks.shape[:2]
    if prompt_embeds is None:
        prompt_embeds = featurizer.encode_prompt(PROMPT_TEMPLATE.format(subject_category))
    fpc = max(1, int(frames_per_call or featurizer.frames_per_call))
    kw = dict(t=t, up_ft_index=up_ft_index, ensemble_size=ensemble_size, generator=generator, prompt_embeds=prompt_embeds)

    def feats(batch):
        ids = [f for f, _ in batch]
        for f in ids:
            if not 0 <= f < F_total:
                raise ValueError(f'frame {f} has no row in pred_tracks [{F_total}, {P}, 2]')
        imgs = _load_batch([p for _, p in batch])
        nz = None
        if noise is not None:
            nz = (torch.stack([noise[f][0] for f in ids]), torch.stack([noise[f][1] for f in ids]))
        return ids, imgs.shape[-2:], featurizer.features(imgs, noise=nz, frames_per_call=fpc, **kw)

    emb, count = None, torch.zeros(P, dtype=torch.float64)
    if is_human:
        # (the reference's confidence_threshold = 0.7 of this branch is never used, extract_semantic_point.py:127)
        for s in range(0, len(frames), fpc):
            ids, (H, W), ft = feats(frames[s:s + fpc])
            r = _round_tracks(tracks[ids])                                             # [n, P, 2]
            seen = (r[..., 0] >= 0) & (r[..., 1] >= 0)
            bad = seen & ((r[..., 0] >= W) | (r[..., 1] >= H))
            if bool(bad.any()):
                f, p = (int(v) for v in bad.nonzero()[0])
                raise ValueError(f'frame {ids[f]} point {p}: {tuple(r[f, p].tolist())} lies outside the {W}x{H} image')
            coords = torch.where(seen[..., None], r, torch.full_like(r, -1)).to(torch.int32)
            vec, _ = ops.dift_sample_points(ft, (H, W), coords.to(ft.device))             # zeros where skipped
            part = vec.double().sum(0).cpu()
            emb = part if emb is None else emb + part
            count += seen.sum(0).double()
    else:
        key = dict(frames)
        if int(keyframe_id) not in key:
            raise ValueError(f'keyframe {keyframe_id} is not among the frames of {frame_dir}')
        kid = int(keyframe_id)
        _, (Hk, Wk), kft = feats([(kid, key[kid])])
        # the keyframe's points, read ONCE before the loop (the reference reads a view of pred_tracks[keyframe] that its
        # loop may already have filtered when the keyframe is not the first file the directory listing returns)
        kp = _round_tracks(tracks[kid])
        src = [[_wrap(int(x), Wk, f'keyframe point {p} x'), _wrap(int(y), Hk, f'keyframe point {p} y')]
               for p, (x, y) in enumerate(kp.tolist())]
        src_vec, _ = ops.dift_sample_points(kft, (Hk, Wk), _coords(src, kft.device))
        query = src_vec[0].contiguous()                                                  # [P, C]
        if vis_dir is not None:
            from PIL import Image
            os.makedirs(vis_dir, exist_ok=True)
            cmap, yx, _ = ops.dift_cosine_map(kft, (Hk, Wk), query)
            img = Image.open(key[kid]).convert('RGB')
            names = {int(i): n for n, i in tap_dict.get('point_name2id', {}).items()}
            for p in range(P):
                heatmap_image(img, cmap[0, p].cpu().numpy(), yx[0, p].tolist(), src[p]).save(
                    os.path.join(vis_dir, f'{kid:05d}_{p:02d}_{names.get(p, p)}.png'))
        for s in range(0, len(frames), fpc):
            ids, (H, W), ft = feats(frames[s:s + fpc])
            r = _round_tracks(tracks[ids])                                             # [n, P, 2]
            outside = (r[..., 0] >= W) | (r[..., 1] >= H)                               # -> [-1, -1], no query
            # a target that rounds negative (an invisible point) is READ from the far edge, as the reference's
            # `tgt_ft[0, :, y, x]` does with a negative Python index; below -W / -H the reference raises, so do we
            low = ~outside & ((r[..., 0] < -W) | (r[..., 1] < -H))
            if bool(low.any()):
                f, p = (int(v) for v in low.nonzero()[0])
                raise ValueError(f'frame {ids[f]} point {p}: {tuple(r[f, p].tolist())} lies outside the {W}x{H} image')
            wrapped = r.clone()
            wrapped[..., 0] = torch.where(r[..., 0] < 0, r[..., 0] + W, r[..., 0])
            wrapped[..., 1] = torch.where(r[..., 1] < 0, r[..., 1] + H, r[..., 1])
            coords = torch.where(outside[..., None], torch.full_like(r, -1), wrapped).to(torch.int32)
            vec, cos = ops.dift_sample_points(ft, (H, W), coords.to(ft.device), query=query, want_cos=True)
            # numpy compares the float32 confidence with the float64 threshold
            keep = ~outside & (cos.cpu().double() >= confidence_threshold)
            part = (vec.double() * keep.to(vec.device, torch.float64)[..., None]).sum(0).cpu()
            emb = part if emb is None else emb + part
            count += keep.sum(0).double()
            for j, f in enumerate(ids):
                tracks[f][~keep[j]] = -1.0
        tap_dict = dict(tap_dict, pred_tracks=tracks)
    if not is_human:
        print('filtered point count:', count.float())
    nz = count > 0
    emb[nz] /= count[nz, None]
    out = dict(tap_dict)
    out['point_embedding'] = emb.float()
    return out
