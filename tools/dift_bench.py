"""Time DIFT point extraction (videoswap_amd.dift.extract_point_embedding, object branch) on seeded synthetic SD-1.5
weights at the dataset shape most configs use: 64 frames of 448x768 (`total_frames: 64`), E = 8, P = 16.

    python tools/dift_bench.py [--frames 64] [--height 448] [--width 768] [--ensemble 8] [--points 16]
                               [--frames_per_call 4] [--out profiles/dift_bench.json]

Prints ONE JSON line: frames/s of the whole extraction (JPEG/PNG decode and host bookkeeping included), the device time
of the VAE encodes, of the UNet calls and of kernels (a) / (b) (hipEvents around each call, after a warm-up pass over
the same shapes), the algorithmic FLOP of the truncated UNet forward (GEMM + attention, ops.FlopCounter) and that
FLOP over the UNet time as a fraction of the 2.5 PF/s dense fp16 MFMA peak.  Kernel (b) is timed once for the
keyframe's P points (the CLI's --vis_dir heat maps), map written.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK_FLOPS = 2.5e15


def _timed_op(ops, name, acc):
    raw = ops._raw[name]

    def run(*a, **k):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        out = raw(*a, **k)
        ev[1].record()
        ev[1].synchronize()
        acc[name] = acc.get(name, 0.0) + ev[0].elapsed_time(ev[1]) / 1e3
        return out
    ops._raw[name] = run
    return raw


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=64)
    ap.add_argument('--height', type=int, default=448)
    ap.add_argument('--width', type=int, default=768)
    ap.add_argument('--ensemble', type=int, default=8)
    ap.add_argument('--points', type=int, default=16)
    ap.add_argument('--frames_per_call', type=int, default=4)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('dift_bench: no GPU (timings exist only on the MI355X)')

    from videoswap_amd import formats, ops
    from videoswap_amd.compat import SD15_SCHEDULER_CONFIG, DDIMScheduler
    from videoswap_amd.dift import SDFeaturizer, extract_point_embedding, list_frames
    from videoswap_amd.synthetic import synth_weights_
    from videoswap_amd.unet import SD15_UNET_CONFIG, AnimateDiffUNet3DModel
    from videoswap_amd.vae import SD15_VAE_CONFIG, AutoencoderKL

    with torch.device('cuda'), torch.no_grad():
        unet = synth_weights_(AnimateDiffUNet3DModel(**SD15_UNET_CONFIG, use_motion_module=False), seed=1234)
        vae = synth_weights_(AutoencoderKL(**SD15_VAE_CONFIG), seed=77)
    fz = SDFeaturizer.from_components(unet, vae, DDIMScheduler(**SD15_SCHEDULER_CONFIG),
                                      frames_per_call=args.frames_per_call)
    H, W, P = args.height, args.width, args.points
    g = torch.Generator().manual_seed(0)
    text = torch.randn(1, 77, 768, generator=g).half()
    with tempfile.TemporaryDirectory() as tmp:
        d = os.path.join(tmp, 'frames')
        formats.synthetic_frames(d, args.frames, W, H, seed=0)
        # synthetic_frames names its files by index: the extraction reads them by int(stem)
        ids = [f for f, _ in list_frames(d)]
        assert ids == list(range(args.frames)), ids[:4]
        tracks = torch.stack([torch.rand(args.frames, P, generator=g) * (W - 1),
                              torch.rand(args.frames, P, generator=g) * (H - 1)], -1)
        tap = {'pred_tracks': tracks, 'point_name2id': {f'p{i}': i for i in range(P)}}
        kw = dict(ensemble_size=args.ensemble, prompt_embeds=text, frames_per_call=args.frames_per_call,
                  generator=torch.Generator(device='cuda').manual_seed(0))

        # warm-up over the same shapes (one full batch of frames + the keyframe call), then the timed pass
        warm = os.path.join(tmp, 'warm')
        os.makedirs(warm)
        for f in range(min(args.frames_per_call, args.frames)):
            src = os.path.join(d, sorted(os.listdir(d))[f])
            os.symlink(src, os.path.join(warm, os.path.basename(src)))
        extract_point_embedding(tap, warm, 0, fz, 'car', False, **kw)
        feat = fz.features(torch.zeros(1, 3, H, W), prompt_embeds=text, ensemble_size=args.ensemble)
        ops.dift_cosine_map(feat, (H, W), torch.randn(P, feat.shape[-1], device='cuda'))
        torch.cuda.synchronize()

        # the UNet's algorithmic FLOP for one frame batch (counted once, outside the timed pass)
        x = torch.zeros(args.frames_per_call * args.ensemble, 4, 1, H // 8, W // 8, dtype=torch.float16, device='cuda')
        ops.FlopCounter.reset(True)
        fz.unet.forward_features(x, 261, text.cuda(), [1])
        ops.FlopCounter.enabled = False
        flop_per_frame = (ops.FlopCounter.gemm + ops.FlopCounter.attention) / args.frames_per_call

        fz.timings = {}
        acc = {}
        saved = {n: _timed_op(ops, n, acc) for n in ('dift_sample_points', 'dift_cosine_map')}
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = extract_point_embedding(tap, d, 0, fz, 'car', False, **kw)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            timings = dict(fz.timings)
            fz.timings = None
            feat = fz.features(torch.zeros(1, 3, H, W), prompt_embeds=text, ensemble_size=args.ensemble)
            ops.dift_cosine_map(feat, (H, W), torch.randn(P, feat.shape[-1], device='cuda'))
        finally:
            ops._raw.update(saved)
        assert out['point_embedding'].shape == (P, feat.shape[-1])

    unet_s = timings['unet']
    flop = flop_per_frame * (args.frames + 1)          # the timed pass runs the keyframe once more for its source vectors
    res = {
        'metric': 'dift_extract_frames_per_s', 'frames': args.frames, 'height': H, 'width': W,
        'ensemble': args.ensemble, 'points': P, 'frames_per_call': args.frames_per_call,
        'frames_per_s': round(args.frames / wall, 3), 'wall_s': round(wall, 3),
        'vae_encode_s': round(timings['vae'], 4), 'unet_s': round(unet_s, 4),
        'kernel_a_s': round(acc.get('dift_sample_points', 0.0), 6),
        'kernel_b_s_keyframe_P_maps': round(acc.get('dift_cosine_map', 0.0), 6),
        'unet_tflop': round(flop / 1e12, 2),
        'unet_mfma_peak_fraction': round(flop / max(unet_s, 1e-9) / PEAK_FLOPS, 4),
        'device': torch.cuda.get_device_name(0),
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
