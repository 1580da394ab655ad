"""DIFT point extraction (videoswap_amd/dift.py, extract_points.py) — host side, no GPU.

The two kernels of csrc/dift.hip are replaced here by stand-ins written in this file (fp32 PyTorch: the ensemble mean,
`F.interpolate(mode='bilinear', align_corners=False)` to image size, indexing and `F.cosine_similarity`), set into
`ops._raw` for the duration of a test; every other op runs on tests/host_emulation.py.  What is checked is the
bookkeeping of extract_semantic_point.py:125-205 against a restatement of that loop in this file: rounding half to
even, skipped / unseen points, the >= W / H filter and the 0.35 threshold of the object branch, reading a negative
target from the far edge, the file that comes out, the CLI and DDIMScheduler.add_noise.
"""
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import host_emulation
from util import ROOT, rel_l2

C_FEAT = 64


# ------------------------------------------------------------------------------------------------
# stand-ins for the two kernels (their contract, include/vsx.h K12)
# ------------------------------------------------------------------------------------------------
def upsampled(feat, size):
    """[N, E, h, w, C] fp16 -> [N, C, H, W] fp32: ensemble mean, then nn.Upsample(size, mode='bilinear')"""
    m = feat.float().mean(1).permute(0, 3, 1, 2)
    return F.interpolate(m, size=tuple(int(s) for s in size), mode='bilinear', align_corners=False)


def standin_sample_points(feat, size, coords, query=None, want_cos=False):
    up = upsampled(feat, size)
    N, P = coords.shape[:2]
    vec = torch.zeros(N, P, up.shape[1])
    cos = torch.zeros(N, P) if want_cos else None
    for n in range(N):
        for p in range(P):
            x, y = (int(v) for v in coords[n, p])
            if x < 0:
                continue
            vec[n, p] = up[n, :, y, x]
            if want_cos:
                q = query[p] if query.dim() == 2 else query[n, p]
                cos[n, p] = F.cosine_similarity(vec[n, p], q.float(), dim=0)
    return vec, cos


def standin_cosine_map(feat, size, query, want_map=True):
    up = upsampled(feat, size)
    N, Q = up.shape[0], query.shape[-2]
    cmap = torch.zeros(N, Q, *up.shape[-2:])
    for n in range(N):
        for q in range(Q):
            qv = query[q] if query.dim() == 2 else query[n, q]
            cmap[n, q] = F.cosine_similarity(qv.float()[:, None, None], up[n], dim=0)
    flat = cmap.flatten(2)
    idx = flat.argmax(-1)
    yx = torch.stack([idx // up.shape[-1], idx % up.shape[-1]], -1).to(torch.int32)
    return (cmap if want_map else None), yx, flat.max(-1).values


@contextlib.contextmanager
def standins():
    from videoswap_amd import ops
    with host_emulation.installed():
        saved = {k: ops._raw.get(k) for k in ('dift_sample_points', 'dift_cosine_map')}
        ops._raw['dift_sample_points'] = standin_sample_points
        ops._raw['dift_cosine_map'] = standin_cosine_map
        try:
            yield
        finally:
            ops._raw.update(saved)


# ------------------------------------------------------------------------------------------------
# a featurizer stand-in: deterministic feature maps per frame (the UNet is covered by tests/test_dift_gpu.py)
# ------------------------------------------------------------------------------------------------
class FakeFeaturizer:
    """features(images) -> [N, E, H/16, W/16, C] fp16: a fixed random base map plus a small per-frame perturbation keyed
    on the image's mean colour, so that cosine similarities at the same place are high and elsewhere low."""

    def __init__(self, E=2, seed=0):
        self.E, self.frames_per_call, self.device = E, 2, torch.device('cpu')
        self.seed = seed
        self.calls = []

    def encode_prompt(self, prompt):
        self.prompt = prompt
        return torch.zeros(1, 77, 8, dtype=torch.float16)

    def features(self, images, noise=None, frames_per_call=None, ensemble_size=None, **kw):
        N, _, H, W = images.shape
        self.calls.append(N)
        g = torch.Generator().manual_seed(self.seed)
        base = torch.randn(self.E, H // 16, W // 16, C_FEAT, generator=g)
        out = []
        for n in range(N):
            key = int(images[n].float().mean().mul(1000).round()) % 1000
            gn = torch.Generator().manual_seed(1000 + key)
            out.append(base + 0.3 * torch.randn(base.shape, generator=gn))
        return torch.stack(out).to(torch.float16)


def write_frames(d, ids, W=128, H=64, ext='.jpg'):
    from PIL import Image
    os.makedirs(d, exist_ok=True)
    for i in ids:
        arr = np.full((H, W, 3), (10 + 20 * i) % 255, dtype=np.uint8)
        arr[:, : W // 2, 1] = 77
        Image.fromarray(arr).save(os.path.join(d, f'{i:05d}{ext}'), quality=100) if ext == '.jpg' else \
            Image.fromarray(arr).save(os.path.join(d, f'{i:05d}{ext}'))


def reference_loop(tap, frame_dir, keyframe, fz, is_human, thr=0.35):
    """extract_semantic_point.py:125-205 restated on the stand-in maps (fp32), with the keyframe points read once."""
    from videoswap_amd.dift import image_tensor, list_frames
    tracks = tap['pred_tracks'].clone().float()
    P = tracks.shape[1]
    emb, cnt = torch.zeros(P, C_FEAT), torch.zeros(P)

    def up(path):
        img = image_tensor(path)
        return upsampled(fz.features(img[None]), img.shape[-2:])[0], img.shape[-2:]

    if is_human:
        for fid, path in list_frames(frame_dir):
            ft, _ = up(path)
            for p, pt in enumerate(tracks[fid]):
                x, y = int(np.round(float(pt[0]))), int(np.round(float(pt[1])))
                if x >= 0 and y >= 0:
                    emb[p] += ft[:, y, x]
                    cnt[p] += 1
    else:
        frames = dict(list_frames(frame_dir))
        kft, _ = up(frames[keyframe])
        kp = tracks[keyframe].clone()
        for fid, path in list_frames(frame_dir):
            ft, (H, W) = up(path)
            for p in range(P):
                sx, sy = np.round(kp[p].numpy())
                tx, ty = np.round(tracks[fid][p].numpy())
                if tx >= W or ty >= H:
                    tracks[fid][p] = torch.tensor([-1, -1])
                    continue
                src = kft[:, int(sy), int(sx)]
                c = F.cosine_similarity(src, ft[:, int(ty), int(tx)], dim=0).numpy()
                if c >= thr:
                    emb[p] += ft[:, int(ty), int(tx)]
                    cnt[p] += 1
                else:
                    tracks[fid][p] = torch.tensor([-1, -1])
    nz = cnt > 0
    emb[nz] /= cnt[nz, None]
    return tracks, emb, cnt


# ------------------------------------------------------------------------------------------------
def test_ddim_add_noise_is_the_forward_diffusion_formula():
    from videoswap_amd.compat import DDIMScheduler, DDPMScheduler
    s = DDIMScheduler(beta_schedule='scaled_linear', beta_start=0.00085, beta_end=0.012, clip_sample=False)
    g = torch.Generator().manual_seed(0)
    x, eps = torch.randn(3, 4, 8, 8, generator=g), torch.randn(3, 4, 8, 8, generator=g)
    a = s.alphas_cumprod[261]
    want = a.sqrt() * x + (1 - a).sqrt() * eps
    assert torch.allclose(s.add_noise(x, eps, torch.tensor([261])), want, atol=1e-6)
    assert torch.allclose(s.add_noise(x, eps, 261), want, atol=1e-6)
    ts = torch.tensor([1, 261, 999])
    d = DDPMScheduler(beta_schedule='scaled_linear', beta_start=0.00085, beta_end=0.012)
    assert torch.allclose(s.add_noise(x, eps, ts), d.add_noise(x, eps, ts), atol=1e-6)


def test_human_branch_rounding_skips_and_unseen(tmp_path):
    from videoswap_amd.dift import extract_point_embedding
    d = str(tmp_path / 'frames')
    write_frames(d, [0, 1, 2])
    tracks = torch.tensor([
        [[2.5, 3.5], [-1.0, 4.0], [-3.0, -3.0], [127.4, 63.4]],      # 2.5 -> 2, 3.5 -> 4 (half to even); x < 0 skipped
        [[3.5, 0.5], [10.0, -0.4], [-1.0, -1.0], [0.0, 0.0]],        # y = -0.4 rounds to -0 -> seen at row 0
        [[100.0, 40.0], [5.0, -2.0], [-1.0, 7.0], [64.5, 31.5]],
    ])
    tap = {'pred_tracks': tracks, 'point_name2id': {'a': 0, 'b': 1, 'c': 2, 'd': 3}}
    fz = FakeFeaturizer()
    with standins():
        out = extract_point_embedding(tap, d, None, fz, 'man', True)
        want_tracks, want_emb, cnt = reference_loop(tap, d, None, FakeFeaturizer(), True)
    assert fz.prompt == 'photo of a man'
    assert fz.calls == [2, 1]                               # frames_per_call = 2: one launch per batch of frames
    assert torch.equal(out['pred_tracks'], tracks)          # the human branch never filters
    assert cnt.tolist() == [3, 1, 0, 3]
    assert torch.equal(out['point_embedding'][2], torch.zeros(C_FEAT))       # never seen: zeros
    assert torch.allclose(out['point_embedding'], want_emb, atol=1e-5)
    assert out['point_embedding'].dtype == torch.float32


def test_human_branch_rejects_coordinates_past_the_image(tmp_path):
    from videoswap_amd.dift import extract_point_embedding
    d = str(tmp_path / 'frames')
    write_frames(d, [0])
    tap = {'pred_tracks': torch.tensor([[[127.6, 3.0]]]), 'point_name2id': {'a': 0}}   # rounds to x = 128 = W
    with standins(), pytest.raises(ValueError, match='outside'):
        extract_point_embedding(tap, d, None, FakeFeaturizer(), 'man', True)


def _object_case(tmp_path):
    d = str(tmp_path / 'frames')
    write_frames(d, [0, 1, 2, 3])
    # keyframe 1.  Frame rows: same place as the keyframe point (kept), elsewhere (filtered), >= W / H (filtered)
    tracks = torch.tensor([
        [[40.0, 20.0], [127.5, 10.0], [8.0, 8.0]],                   # 127.5 rounds to 128 = W -> [-1, -1]
        [[40.0, 20.0], [90.0, 40.0], [8.0, 8.0]],
        [[40.4, 19.6], [10.0, 50.0], [-1.0, -1.0]],                  # -1 -> read at the far edge (x = W-1, y = H-1)
        [[100.0, 5.0], [90.0, 63.5], [8.0, 8.0]],                     # 63.5 rounds to 64 = H -> [-1, -1]
    ])
    return d, {'pred_tracks': tracks, 'point_name2id': {'p0': 0, 'p1': 1, 'p2': 2}}


def test_object_branch_filter_threshold_and_wrap(tmp_path):
    from videoswap_amd.dift import extract_point_embedding
    d, tap = _object_case(tmp_path)
    before = tap['pred_tracks'].clone()
    with standins():
        out = extract_point_embedding(tap, d, 1, FakeFeaturizer(), 'car', False)
        want_tracks, want_emb, cnt = reference_loop(tap, d, 1, FakeFeaturizer(), False)
    assert torch.equal(tap['pred_tracks'], before)                       # the input is not modified
    assert torch.equal(out['pred_tracks'], want_tracks)
    assert torch.allclose(out['point_embedding'], want_emb, atol=1e-5)
    got = out['pred_tracks']
    assert got[0, 1].tolist() == [-1, -1] and got[3, 1].tolist() == [-1, -1]     # >= W, >= H
    assert got[1].tolist() == before[1].tolist()                         # the keyframe matches itself
    kept = (got[..., 0] >= 0).sum().item()
    assert 0 < kept < got.shape[0] * got.shape[1]                        # some kept, some filtered
    assert cnt[1] == 1                                                   # p1: only the keyframe itself


def test_object_branch_reads_negative_targets_from_the_far_edge(tmp_path):
    """a target at (-1, -1) is the reference's `tgt_ft[0, :, -1, -1]`: the bottom-right pixel of the upsampled map"""
    from videoswap_amd.dift import extract_point_embedding, image_tensor
    d = str(tmp_path / 'frames')
    write_frames(d, [0, 1])
    tracks = torch.tensor([[[127.0, 63.0]], [[-1.0, -1.0]]])
    tap = {'pred_tracks': tracks, 'point_name2id': {'p': 0}}
    fz = FakeFeaturizer()
    with standins():
        out = extract_point_embedding(tap, d, 0, fz, 'car', False, confidence_threshold=-2.0)
        f1 = upsampled(fz.features(image_tensor(os.path.join(d, '00001.jpg'))[None]), (64, 128))[0]
        f0 = upsampled(fz.features(image_tensor(os.path.join(d, '00000.jpg'))[None]), (64, 128))[0]
    assert out['pred_tracks'][1].tolist() == [[-1.0, -1.0]]           # unchanged: kept at threshold -2
    want = (f0[:, 63, 127] + f1[:, -1, -1]) / 2
    assert torch.allclose(out['point_embedding'][0], want, atol=1e-5)


def test_object_branch_keyframe_points_are_read_before_the_loop(tmp_path):
    """frame 0 is listed first and filters keyframe 1's own row in the reference only if the keyframe row were written
    (it is not: rows of OTHER frames are filtered) — here the keyframe row is filtered itself (>= W), and the source
    vectors must still come from the keyframe's original points"""
    from videoswap_amd.dift import extract_point_embedding
    d = str(tmp_path / 'frames')
    write_frames(d, [0, 1])
    tracks = torch.tensor([[[30.0, 30.0]], [[30.0, 30.0]]])
    tap = {'pred_tracks': tracks, 'point_name2id': {'p': 0}}
    with standins():
        a = extract_point_embedding(tap, d, 0, FakeFeaturizer(), 'car', False)
        os.rename(os.path.join(d, '00000.jpg'), os.path.join(d, '00002.jpg'))  # keyframe now listed last
        tap2 = {'pred_tracks': torch.tensor([[[30.0, 30.0]], [[30.0, 30.0]], [[30.0, 30.0]]]), 'point_name2id': {'p': 0}}
        b = extract_point_embedding(tap2, d, 2, FakeFeaturizer(), 'car', False)
    assert a['pred_tracks'][0].tolist() == [[30.0, 30.0]]
    assert torch.allclose(a['point_embedding'], b['point_embedding'], atol=1e-6)


def test_output_roundtrips_through_load_tap_and_the_dataset(tmp_path):
    from videoswap_amd import formats
    from videoswap_amd.data import SingleVideoPointDataset
    from videoswap_amd.dift import extract_point_embedding
    d, tap = _object_case(tmp_path)
    with standins():
        out = extract_point_embedding(tap, d, 1, FakeFeaturizer(), 'car', False)
    path = str(tmp_path / 'TAP.pth')
    formats.save_tap(path, out['pred_tracks'], out['point_embedding'], out['point_name2id'])
    back = formats.load_tap(path)
    assert torch.equal(back['pred_tracks'], out['pred_tracks'])
    assert torch.equal(back['point_embedding'], out['point_embedding'])
    assert back['point_name2id'] == tap['point_name2id']
    ds = SingleVideoPointDataset({'path': d, 'total_frames': 3, 'num_frames': 2, 'prompt': 'a car',
                                  'video_transform': [{'type': 'ToTensor'}], 'tap_path': path})
    item = ds[0]
    assert item['point_embedding'].shape == (3, C_FEAT)
    assert torch.equal(item['pred_tracks'], out['pred_tracks'][ds.select_id])


def test_load_tracks_ignores_embeddings_and_load_tap_still_requires_them(tmp_path):
    from videoswap_amd import formats
    p = str(tmp_path / 'tracks.pth')
    torch.save({'pred_tracks': torch.zeros(2, 3, 2), 'point_name2id': {'a': 2}, 'point_embedding': torch.ones(3, 5)}, p)
    t = formats.load_tracks(p)
    assert set(t) == {'pred_tracks', 'point_name2id'}
    q = str(tmp_path / 'only_tracks.pth')
    torch.save({'pred_tracks': torch.zeros(2, 3, 2), 'point_name2id': {'a': 2}}, q)
    assert formats.load_tracks(q)['point_name2id'] == {'a': 2}
    with pytest.raises(formats.FormatError):
        formats.load_tap(q)
    torch.save({'pred_tracks': torch.zeros(2, 3, 2), 'point_name2id': {'a': 3}}, q)
    with pytest.raises(formats.FormatError):
        formats.load_tracks(q)


def test_cli_arguments(tmp_path):
    from videoswap_amd.extract_points import parse_args
    base = ['--frame_dir', 'f', '--tracks', 't.pth', '--model_id', 'sd', '--subject_category', 'car', '--save_path', 'o.pth']
    a = parse_args(base + ['--keyframe_annotation_path', 'ann/00035.json'])
    assert a.keyframe == 35 and a.is_human is False and a.frames_per_call == 4 and a.seed == 0 and a.vis_dir is None
    a = parse_args(base + ['--keyframe', '7', '--frames_per_call', '2', '--seed', '3', '--vis_dir', 'v'])
    assert (a.keyframe, a.frames_per_call, a.seed, a.vis_dir) == (7, 2, 3, 'v')
    a = parse_args(base + ['--is_human', 'true'])
    assert a.is_human is True and a.keyframe is None
    for bad in (base, base + ['--keyframe_annotation_path', 'x/abc.json'], base + ['--keyframe', '1', '--frames_per_call', '0']):
        with pytest.raises(SystemExit):
            parse_args(bad)
    with pytest.raises(SystemExit):
        parse_args(base + ['--keyframe', '1', '--keyframe_annotation_path', 'a/1.json'])
    with pytest.raises(SystemExit):
        parse_args(base + ['--is_human', 'maybe'])


def test_cli_run_writes_a_tap_file(tmp_path):
    from videoswap_amd import formats
    from videoswap_amd.extract_points import parse_args, run
    d, tap = _object_case(tmp_path)
    tp = str(tmp_path / 'in.pth')
    torch.save(dict(tap, point_embedding=torch.ones(3, 9)), tp)
    out_path = str(tmp_path / 'out' / 'TAP.pth')
    vis = str(tmp_path / 'vis')
    args = parse_args(['--frame_dir', d, '--tracks', tp, '--model_id', 'unused', '--subject_category', 'car',
                       '--keyframe', '1', '--save_path', out_path, '--vis_dir', vis])
    with standins():
        run(args, featurizer=FakeFeaturizer())
    back = formats.load_tap(out_path)
    assert back['point_embedding'].shape == (3, C_FEAT)
    assert sorted(os.listdir(vis)) == ['00001_00_p0.png', '00001_01_p1.png', '00001_02_p2.png']


def test_frame_listing_and_image_tensor(tmp_path):
    from PIL import Image
    from videoswap_amd.dift import image_tensor, list_frames
    d = tmp_path / 'f'
    write_frames(str(d), [3, 1], ext='.png')
    (d / 'notes.txt').write_text('x')
    assert [f for f, _ in list_frames(str(d))] == [1, 3]
    img = Image.open(d / '00001.png')
    t = image_tensor(img)
    want = (torch.from_numpy(np.array(img)).permute(2, 0, 1) / 255.0 - 0.5) * 2
    assert t.shape == (3, 64, 128) and torch.equal(t, want)
    (d / 'x.png').write_bytes(b'')
    with pytest.raises(ValueError):
        list_frames(str(d))


def _tiny_featurizer():
    from oracle import unet3d
    from oracle import vae as ovae
    from videoswap_amd.compat import DDIMScheduler
    from videoswap_amd.dift import SDFeaturizer
    from videoswap_amd.unet import AnimateDiffUNet3DModel
    from videoswap_amd.vae import AutoencoderKL
    cfg = dict(unet3d.SD15_UNET_CONFIG, block_out_channels=(64, 128, 256, 256), cross_attention_dim=64)
    unet = AnimateDiffUNet3DModel(**cfg, use_motion_module=False)
    ora = unet3d.AnimateDiffUNet3DModel(**cfg, use_motion_module=False).eval()
    unet3d.synth_weights_(ora, seed=5)
    unet.load_state_dict(ora.state_dict())
    vae = AutoencoderKL(**ovae.tiny_vae_config())
    vae.load_state_dict(ovae.synth_weights_(ovae.AutoencoderKL(**ovae.tiny_vae_config()), seed=6).state_dict(), strict=False)
    sched = DDIMScheduler(beta_schedule='scaled_linear', beta_start=0.00085, beta_end=0.012, clip_sample=False)
    return SDFeaturizer.from_components(unet, vae, sched, device='cpu', frames_per_call=1)


def test_featurizer_wiring_on_the_host_mirror():
    """SDFeaturizer + forward_features on tests/host_emulation.py: shapes, the truncation point, injected noise"""
    fz = _tiny_featurizer()
    g = torch.Generator().manual_seed(0)
    imgs = torch.rand(2, 3, 64, 128, generator=g) * 2 - 1
    E = 2
    noise = (torch.randn(2, E, 4, 8, 16, generator=g), torch.randn(2, E, 4, 8, 16, generator=g))
    text = torch.randn(1, 77, 64, generator=g)
    with host_emulation.installed():
        ft = fz.features(imgs, prompt_embeds=text, ensemble_size=E, noise=noise, frames_per_call=1)
        ft2 = fz.features(imgs, prompt_embeds=text, ensemble_size=E, noise=noise, frames_per_call=2)
        one = fz.forward(imgs[1], None, ensemble_size=E, prompt_embeds=text, noise=(noise[0][1], noise[1][1]))
        x = torch.randn(2, 4, 1, 8, 16, generator=g).half()
        taps = fz.unet.forward_features(x, 261, text.half(), [0, 1, 3])
    assert ft.shape == (2, E, 4, 8, 256) and ft.dtype == torch.float16          # up block 1: 1/16 of the image side
    assert rel_l2(ft2, ft) < 1e-2                                               # batching: the same up to fp16 roundings
    assert one.shape == (1, 256, 4, 8) and rel_l2(one.vsx_ensemble, ft[1:2]) < 1e-2
    assert torch.allclose(one[0], one.vsx_ensemble[0].float().mean(0).permute(2, 0, 1))
    assert sorted(taps) == [0, 1, 3]
    assert taps[0].shape == (2, 2, 4, 256) and taps[1].shape == (2, 4, 8, 256) and taps[3].shape == (2, 8, 16, 64)
    with pytest.raises(ValueError, match='multiples of 64'):
        fz.features(torch.zeros(1, 3, 64, 96), prompt_embeds=text)
    with pytest.raises(ValueError):
        fz.unet.forward_features(x, 261, text.half(), [4])


def test_dift_util_shim_names():
    code = ('import sys; sys.path.insert(0, %r); from videoswap.utils.dift_util import SDFeaturizer, DIFT_Demo; '
            'from videoswap_amd import dift; assert SDFeaturizer is dift.SDFeaturizer and DIFT_Demo is dift.DIFTDemo'
            % os.path.join(ROOT, 'videoswap_amd', 'shims'))
    r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True, text=True,
                       env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stderr
