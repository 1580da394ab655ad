"""DIFT point extraction on the MI355X: the two kernels of csrc/dift.hip against fp32 PyTorch on the same fp16 input,
AnimateDiffUNet3DModel.forward_features at SD-1.5 width against the fp32 oracle UNet driven block by block, and the
whole extraction (both branches) against the fp32 restatement of extract_semantic_point.py in tests/test_dift.py."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from util import cosine, rel_l2

pytestmark = pytest.mark.gpu


def _dense(feat, size):
    """[N, E, h, w, C] fp16 -> [N, C, H, W] fp32 (mean over E, then nn.Upsample bilinear)"""
    m = feat.float().mean(1).permute(0, 3, 1, 2)
    return F.interpolate(m, size=size, mode='bilinear', align_corners=False)


def _points(H, W, P, g):
    pts = [[0, 0], [W - 1, 0], [0, H - 1], [W - 1, H - 1], [W // 2, 0], [0, H // 2], [W - 1, H // 2], [W // 2, H - 1]]
    while len(pts) < P:
        pts.append([int(torch.randint(0, W, (1,), generator=g)), int(torch.randint(0, H, (1,), generator=g))])
    return pts[:P]


@pytest.mark.parametrize('h,w,H,W,E,C', [(28, 48, 448, 768, 8, 1280), (28, 48, 448, 768, 1, 1280),
                                         (32, 32, 512, 512, 8, 1280), (13, 21, 203, 333, 1, 320)])
def test_sample_points_matches_upsample_and_index(h, w, H, W, E, C):
    from videoswap_amd import ops
    g = torch.Generator().manual_seed(h * w + E)
    N, P = 2, 12
    feat = torch.randn(N, E, h, w, C, generator=g).half().cuda()
    coords = torch.tensor([_points(H, W, P, g) for _ in range(N)], dtype=torch.int32)
    coords[0, 9] = torch.tensor([-1, 5])                       # skipped
    coords[1, 10] = torch.tensor([-3, -3])
    query = torch.randn(P, C, generator=g).cuda()
    vec, cos = ops.dift_sample_points(feat, (H, W), coords.cuda(), query=query, want_cos=True)
    vq, cq = ops.dift_sample_points(feat, (H, W), coords.cuda(), query=torch.stack([query, -query]).contiguous(),
                                    want_cos=True)
    plain, none = ops.dift_sample_points(feat, (H, W), coords.cuda())
    torch.cuda.synchronize()
    up = _dense(feat, (H, W))
    for n in range(N):
        for p in range(P):
            x, y = (int(v) for v in coords[n, p])
            if x < 0:
                assert float(vec[n, p].abs().max()) == 0 and float(cos[n, p]) == 0
                continue
            ref = up[n, :, y, x]
            err = float((vec[n, p] - ref).abs().max())
            assert err <= 1e-5 * float(ref.norm()), (n, p, x, y, err)
            rc = float(F.cosine_similarity(ref, query[p], dim=0))
            assert abs(float(cos[n, p]) - rc) <= 1e-5
            assert abs(float(cq[n, p]) - (rc if n == 0 else -rc)) <= 1e-5          # [N, P, C] queries
    assert torch.equal(plain, vec) and torch.equal(vq, vec) and none is None


@pytest.mark.parametrize('h,w,H,W,E,Q', [(28, 48, 448, 768, 8, 3), (13, 21, 203, 333, 2, 2)])
def test_cosine_map_matches_the_dense_map(h, w, H, W, E, Q):
    from videoswap_amd import ops
    g = torch.Generator().manual_seed(7 + h)
    N, C = 2, 1280
    base = torch.randn(1, 1, h, w, C, generator=g)
    feat = (base + 0.5 * torch.randn(N, E, h, w, C, generator=g)).half().cuda()   # correlated neighbours / frames
    query = _dense(feat[:1], (H, W))[0, :, [5, H // 2, H - 1][:Q], [7, W - 1, 0][:Q]].t().contiguous()
    cmap, yx, val = ops.dift_cosine_map(feat, (H, W), query)
    none, yx2, val2 = ops.dift_cosine_map(feat, (H, W), query, want_map=False)
    torch.cuda.synchronize()
    assert none is None and torch.equal(yx, yx2) and torch.equal(val, val2)
    up = _dense(feat, (H, W))
    for n in range(N):
        for q in range(Q):
            ref = F.cosine_similarity(query[q][:, None, None], up[n], dim=0)
            assert float((cmap[n, q] - ref).abs().max()) <= 2e-4
            y, x = (int(v) for v in yx[n, q])
            assert float(val[n, q]) == float(cmap[n, q, y, x])
            assert float(ref.max()) - float(ref[y, x]) <= 2e-4
            flat = int(cmap[n, q].flatten().argmax())                 # row-major first among equal values
            assert (y, x) == np.unravel_index(flat, (H, W))


# ------------------------------------------------------------------------------------------------
# forward_features at SD-1.5 width (the featurizer's 2-D UNet) against the fp32 oracle
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def unets():
    from oracle import unet3d
    from videoswap_amd.synthetic import synth_weights_
    from videoswap_amd.unet import AnimateDiffUNet3DModel
    cfg = dict(unet3d.SD15_UNET_CONFIG, use_motion_module=False)
    with torch.device('cuda'):
        prod = AnimateDiffUNet3DModel(**cfg)
        ora = unet3d.AnimateDiffUNet3DModel(**cfg).eval()
    prod = synth_weights_(prod, seed=4321).half().eval()
    missing, unexpected = ora.load_state_dict({k: v.float() for k, v in prod.state_dict().items()}, strict=True)
    assert not missing and not unexpected
    return prod, ora, copy.deepcopy(ora).half()


@torch.no_grad()
def _oracle_taps(ora, x, t, text, upto):
    """oracle.unet3d driven block by block: conv_in, down, mid, up 0 ... upto -> {i: [B, C, F, h, w]}"""
    dt = next(ora.parameters()).dtype
    x, text = x.to(dt), text.to(dt)
    emb = ora.time_embedding(ora.time_proj(torch.tensor([t], device=x.device).expand(x.shape[0])).to(dt))
    h = ora.conv_in(x)
    skips = (h,)
    for blk in ora.down_blocks:
        h, res = blk(h, temb=emb, encoder_hidden_states=text)
        skips += res
    h = ora.mid_block(h, emb, encoder_hidden_states=text)
    out = {}
    for i, blk in enumerate(ora.up_blocks[:upto + 1]):
        n = len(blk.resnets)
        res, skips = skips[-n:], skips[:-n]
        h = blk(h, res, temb=emb, encoder_hidden_states=text)
        out[i] = h.float()
    return out


def test_forward_features_matches_the_oracle_and_forward_is_unchanged(unets):
    prod, ora, ora_h = unets
    g = torch.Generator().manual_seed(3)
    B = 3
    x = torch.randn(B, 4, 1, 32, 48, generator=g).cuda()
    text = torch.randn(1, 77, 768, generator=g).cuda()
    taps = prod.forward_features(x.half(), 261, text.half(), [0, 1])
    want = _oracle_taps(ora, x, 261, text.expand(B, -1, -1), 1)
    yard = _oracle_taps(ora_h, x, 261, text.expand(B, -1, -1), 1)
    for i, side in ((0, (8, 12)), (1, (16, 24))):
        got = taps[i].float().view(B, 1, *taps[i].shape[1:]).permute(0, 4, 1, 2, 3)
        assert tuple(taps[i].shape) == (B,) + side + (1280,)
        e, y = rel_l2(got, want[i]), rel_l2(yard[i], want[i])
        print(f'up block {i}: rel-L2 {e:.2e} (fp16 oracle {y:.2e}), cosine {cosine(got, want[i]):.6f}')
        assert e <= 2 * y and cosine(got, want[i]) >= 0.999
    # forward itself on the same weights
    with torch.no_grad():
        out = prod(x.half(), 261, text.half().expand(B, -1, -1).contiguous()).sample.float()
        ref = ora(x, 261, text.expand(B, -1, -1)).sample.float()
        yref = ora_h(x.half(), 261, text.half().expand(B, -1, -1)).sample.float()
    e, y = rel_l2(out, ref), rel_l2(yref, ref)
    print(f'forward: rel-L2 {e:.2e} (fp16 oracle {y:.2e})')
    assert e <= 2 * y


# ------------------------------------------------------------------------------------------------
# end to end: both branches, injected noise and prompt embedding, vs the fp32 restatement
# ------------------------------------------------------------------------------------------------
def _frames(d, n, H, W):
    import os
    from PIL import Image
    g = torch.Generator().manual_seed(11)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing='ij')
    base = torch.stack([xx, yy, (xx + yy) / 2]) * 200 + 20
    os.makedirs(d, exist_ok=True)
    for i in range(n):
        img = (base + 25 * torch.randn(3, H, W, generator=g) * (i > 0)).clamp(0, 255).byte()
        Image.fromarray(img.permute(1, 2, 0).numpy()).save(os.path.join(d, f'{i:05d}.png'))


def test_extraction_end_to_end_both_branches(unets, tmp_path):
    from oracle import vae as ovae
    from videoswap_amd.compat import DDIMScheduler
    from videoswap_amd.dift import SDFeaturizer, extract_point_embedding, image_tensor, list_frames
    from videoswap_amd.vae import AutoencoderKL
    prod, ora, _ = unets
    H, W, E, nf = 256, 384, 4, 3
    d = str(tmp_path / 'frames')
    _frames(d, nf, H, W)
    ovae_m = ovae.synth_weights_(ovae.AutoencoderKL(**ovae.tiny_vae_config()), seed=9).cuda().eval()
    pvae = AutoencoderKL(**ovae.tiny_vae_config())
    pvae.load_state_dict(ovae_m.state_dict(), strict=False)
    sched = DDIMScheduler(beta_schedule='scaled_linear', beta_start=0.00085, beta_end=0.012, clip_sample=False)
    fz = SDFeaturizer.from_components(prod, pvae, sched, frames_per_call=2)
    g = torch.Generator().manual_seed(5)
    noise = {i: (torch.randn(E, 4, H // 8, W // 8, generator=g), torch.randn(E, 4, H // 8, W // 8, generator=g))
             for i in range(nf)}
    text = torch.randn(1, 77, 768, generator=g)

    # fp32 oracle maps [C, H, W] per frame: oracle VAE + oracle UNet (fp32), ensemble mean, upsample
    a = sched.alphas_cumprod[261]
    up = {}
    with torch.no_grad():
        for fid, path in list_frames(d):
            img = image_tensor(path)[None].cuda().expand(E, -1, -1, -1)
            z = ovae_m.encode_sample(img, noise[fid][0].cuda()) * 0.18215
            z = a.sqrt() * z + (1 - a).sqrt() * noise[fid][1].cuda()
            ft = _oracle_taps(ora, z[:, :, None], 261, text.cuda().expand(E, -1, -1), 1)[1][:, :, 0]   # [E, C, h, w]
            up[fid] = F.interpolate(ft.mean(0, keepdim=True), size=(H, W), mode='bilinear', align_corners=False)[0].cpu()

    def oracle_loop(tap, keyframe, is_human):
        tracks = tap['pred_tracks'].clone().float()
        P = tracks.shape[1]
        emb, cnt = torch.zeros(P, 1280), torch.zeros(P)
        kp = None if is_human else tracks[keyframe].clone()
        for fid, _ in list_frames(d):
            for p in range(P):
                tx, ty = (int(v) for v in np.round(tracks[fid][p].numpy()))
                if is_human:
                    if tx >= 0 and ty >= 0:
                        emb[p] += up[fid][:, ty, tx]
                        cnt[p] += 1
                    continue
                if tx >= W or ty >= H:
                    tracks[fid][p] = -1
                    continue
                sx, sy = (int(v) for v in np.round(kp[p].numpy()))
                c = float(F.cosine_similarity(up[keyframe][:, sy, sx], up[fid][:, ty, tx], dim=0))
                if c >= 0.35:
                    emb[p] += up[fid][:, ty, tx]
                    cnt[p] += 1
                else:
                    tracks[fid][p] = -1
        nz = cnt > 0
        emb[nz] /= cnt[nz, None]
        return tracks, emb, cnt

    # object-branch tracks chosen on the oracle's own cosine maps: kept targets above 0.40, filtered ones below 0.30
    kid, P = 0, 4
    src = [[40, 30], [200, 128], [350, 200], [100, 220]]
    tracks = torch.zeros(nf, P, 2)
    tracks[kid] = torch.tensor(src, dtype=torch.float32)
    for fid in range(1, nf):
        for p, (sx, sy) in enumerate(src):
            cmap = F.cosine_similarity(up[kid][:, sy, sx][:, None, None], up[fid], dim=0)
            hi = (cmap > 0.40).nonzero()
            lo = (cmap < 0.30).nonzero()
            pick = hi if (p % 2 == 0 or len(lo) == 0) else lo
            assert len(pick), f'no target pixel with a margin around 0.35 (point {p}, frame {fid})'
            y, x = (int(v) for v in pick[len(pick) // 2])
            tracks[fid, p] = torch.tensor([x + 0.4, y - 0.4])
    tracks[1, 3] = torch.tensor([W + 0.0, 10.0])                     # >= W: filtered before any query
    tracks[2, 2] = torch.tensor([-1.0, -1.0])                        # read from the far edge
    c = F.cosine_similarity(up[kid][:, src[2][1], src[2][0]], up[2][:, -1, -1], dim=0)
    if abs(float(c) - 0.35) < 0.02:
        tracks[2, 2] = torch.tensor([5.0, 5.0])
    tap = {'pred_tracks': tracks, 'point_name2id': {f'p{i}': i for i in range(P)}}
    out = extract_point_embedding(tap, d, kid, fz, 'car', False, ensemble_size=E, prompt_embeds=text, noise=noise)
    want_tracks, want_emb, cnt = oracle_loop(tap, kid, False)
    assert torch.equal(out['pred_tracks'], want_tracks)
    kept = want_tracks[1:, :, 0] >= 0
    assert bool(kept.any()) and not bool(kept.all())
    for p in range(P):
        assert cosine(out['point_embedding'][p], want_emb[p]) >= 0.999, p

    # human branch: same frames, negatives skipped
    ht = tracks.clone()
    ht[1, 0] = torch.tensor([-2.0, 40.0])
    ht[2, 1] = torch.tensor([30.0, -0.6])
    ht[2, 3] = torch.tensor([12.5, 7.5])
    tap = {'pred_tracks': ht, 'point_name2id': {f'p{i}': i for i in range(P)}}
    tap['pred_tracks'][1, 3] = torch.tensor([20.0, 20.0])
    hout = extract_point_embedding(tap, d, None, fz, 'man', True, ensemble_size=E, prompt_embeds=text, noise=noise)
    _, hwant, _ = oracle_loop(tap, None, True)
    assert torch.equal(hout['pred_tracks'], tap['pred_tracks'])
    for p in range(P):
        assert cosine(hout['point_embedding'][p], hwant[p]) >= 0.999, p
