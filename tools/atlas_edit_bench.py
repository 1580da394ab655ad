"""A first reading of the edit path (ops.atlas_edit: csrc/atlas_edit.hip K15, and atlas.edit_atlas) at the sizes of the
reference's configs: one 768 x 448 frame (344 064 rows) through the mapping networks of tools/atlas_render_bench.py
(hidden 256; untrained, at the nn.Linear default initialisation) and two random 1000 x 1000 RGB textures, the foreground
over [0, 1]^2 and the background over [-1, 0]^2.

    python tools/atlas_edit_bench.py [--reps 20] [--out profiles/atlas_edit_first.json]

Variants, timed in rotation (every repetition runs each variant once, in an order that shifts by one per repetition, so
that drift of the clocks and of the shared host meets all of them alike), each by hipEvents around the call, medians
after a warm-up of the same shapes:
  op           ops.atlas_edit alone on the frame's uv / alpha (one launch),
  op_random_uv the same on uv drawn uniformly over (and a little beyond) both boxes: gathers all over the two 12 MB textures,
               where the networks' own uv are smooth in the pixel position,
  op_masks     the same with both mask images, zeroed inside the timed call (two 4 MB fills): a row reads each of its eight
               cells and issues the integer atomic only where its value is larger,
  op_rgba      the same with two RGBA overlays (the base colours are inputs here),
  torch        the same step written as PyTorch-ROCm tensor ops in this process (gathers, about a dozen [N, 3] temporaries),
  chunk        atlas.edit_atlas on the frame: FG_UV_Mapping, BG_UV_Mapping, F_Alpha, ops.atlas_edit and the torch glue.
The share the op takes is op / chunk.  Bytes per row are the algorithm's streaming traffic (two uv pairs, alpha, three
[N, 3] outputs, one byte of relevance: 57 B; the texture gathers are not counted), so the GB/s is a lower figure than
what the memory system moves.  There is no threshold: this is a first measurement.  Prints ONE JSON line.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from atlas_render_bench import MODELS, RES_X, RES_Y  # noqa: E402

R = 1000
BYTES_PER_ROW = 2 * 8 + 4 + 3 * 12 + 1


def torch_layer(uv, tex, box, shift):
    """one layer of include/vsx.h K15 as tensor ops -> (colour [N, 3], relevant [N])"""
    minx, miny, ps = box
    n = tex.shape[0]
    q = uv * 0.5 + shift
    px, py = (q[:, 0] - minx) * ps, (q[:, 1] - miny) * ps
    fx, fy = torch.floor(px), torch.floor(py)
    relevant = (fx >= 0) & (fy >= 0) & (torch.ceil(px) < n) & (torch.ceil(py) < n)
    x0, y0 = fx.clamp(0, n - 1).long(), fy.clamp(0, n - 1).long()
    x1, y1 = (x0 + 1).clamp(max=n - 1), (y0 + 1).clamp(max=n - 1)
    wx1, wx0, wy1, wy0 = x1 - px, px - x0, y1 - py, py - y0
    flat = tex.view(n * n, -1)
    col = flat[y0 * n + x0] * (wx1 * wy1).unsqueeze(1) + flat[y1 * n + x0] * (wx1 * wy0).unsqueeze(1) \
        + flat[y0 * n + x1] * (wx0 * wy1).unsqueeze(1) + flat[y1 * n + x1] * (wx0 * wy0).unsqueeze(1)
    return col, relevant


def torch_edit(uv_fg, uv_bg, alpha, tex_fg, box_fg, tex_bg, box_bg):
    cf, rf = torch_layer(uv_fg, tex_fg, box_fg, 0.5)
    cb, rb = torch_layer(uv_bg, tex_bg, box_bg, -0.5)
    a = alpha.unsqueeze(1)
    zero = torch.zeros_like(cf)
    fg = torch.where(rf.unsqueeze(1), cf * a, zero)
    bg = torch.where(rb.unsqueeze(1), cb, zero)
    edit = fg + torch.where(rb.unsqueeze(1), cb * (1.0 - a), zero)
    return edit, fg, bg, rf.to(torch.uint8) | (rb.to(torch.uint8) << 1)


def rotated_medians(variants, reps, warmup=3):
    """{name: (median, min, max) ms}: every repetition times each variant once, the order shifted by one per repetition"""
    names = list(variants)
    for _ in range(warmup):
        for n in names:
            variants[n]()
    torch.cuda.synchronize()
    times = {n: [] for n in names}
    for r in range(reps):
        for k in range(len(names)):
            n = names[(k + r) % len(names)]
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            variants[n]()
            ev[1].record()
            ev[1].synchronize()
            times[n].append(ev[0].elapsed_time(ev[1]))
    return {n: (statistics.median(t), min(t), max(t)) for n, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('atlas_edit_bench needs the GPU: nothing here can be timed on the CPU')
    from videoswap_amd import atlas, ops
    torch.manual_seed(0)
    nets = {n: atlas.build_network(kw).cuda() for n, kw in MODELS.items()}
    N = RES_X * RES_Y
    tex_fg, tex_bg = torch.rand(R, R, 3, device='cuda'), torch.rand(R, R, 3, device='cuda')
    rgba_fg, rgba_bg = torch.rand(R, R, 4, device='cuda'), torch.rand(R, R, 4, device='cuda')
    box_fg, box_bg = atlas.texture_box(0, 0, 1, R), atlas.texture_box(-1, -1, 1, R)
    with torch.no_grad():
        first = atlas.render_atlas(nets, RES_X, RES_Y, 72, frames=[0])
        uv_fg, uv_bg = first['uv_fg'].reshape(N, 2).contiguous(), first['uv_bg'].reshape(N, 2).contiguous()
        alpha = first['alpha'].reshape(N).contiguous()
        base = torch.rand(N, 3, device='cuda')
        ruv_fg, ruv_bg = torch.rand(N, 2, device='cuda') * 2.2 - 1.1, torch.rand(N, 2, device='cuda') * 2.2 - 1.1
        masks = (torch.zeros(R, R, device='cuda'), torch.zeros(R, R, device='cuda'))
        got = ops.atlas_edit(uv_fg, uv_bg, alpha, tex_fg, box_fg, tex_bg, box_bg)
        ref = torch_edit(uv_fg, uv_bg, alpha, tex_fg, box_fg, tex_bg, box_bg)
        diff = max(float((g - r).abs().max()) for g, r in zip(got[:3], ref[:3]))
        rel_equal = bool(torch.equal(got[3], ref[3]))
        def op_masks():
            masks[0].zero_()
            masks[1].zero_()
            return ops.atlas_edit(uv_fg, uv_bg, alpha, tex_fg, box_fg, tex_bg, box_bg, masks=masks)

        variants = {
            'op': lambda: ops.atlas_edit(uv_fg, uv_bg, alpha, tex_fg, box_fg, tex_bg, box_bg),
            'op_random_uv': lambda: ops.atlas_edit(ruv_fg, ruv_bg, alpha, tex_fg, box_fg, tex_bg, box_bg),
            'op_masks': op_masks,
            'op_rgba': lambda: ops.atlas_edit(uv_fg, uv_bg, alpha, rgba_fg, box_fg, rgba_bg, box_bg, base_fg=base, base_bg=base),
            'torch': lambda: torch_edit(uv_fg, uv_bg, alpha, tex_fg, box_fg, tex_bg, box_bg),
            'chunk': lambda: atlas.edit_atlas(nets, RES_X, RES_Y, 72, tex_fg, box_fg, tex_bg, box_bg, frames=[0]),
        }
        ms = rotated_medians(variants, args.reps)
    rel = got[3]
    result = {'metric': 'atlas_edit', 'device': torch.cuda.get_device_name(0), 'rows_per_frame': N, 'reps': args.reps,
              'texture_resolution': R, 'texture_MB_each': round(R * R * 3 * 4 / 1e6, 2), 'streamed_bytes_per_row': BYTES_PER_ROW,
              'relevant_share_fg': round(float(((rel & 1) != 0).float().mean()), 4),
              'relevant_share_bg': round(float(((rel & 2) != 0).float().mean()), 4),
              'mask_cells_marked_fg_bg': [int((masks[0] > 0).sum()), int((masks[1] > 0).sum())],
              'max_abs_diff_op_vs_torch': diff, 'relevant_equal_op_vs_torch': rel_equal,
              'ms': {n: {'median': round(v[0], 4), 'min': round(v[1], 4), 'max': round(v[2], 4)} for n, v in ms.items()},
              'op_streamed_GB_per_s': round(N * BYTES_PER_ROW / ms['op'][0] / 1e6, 1),
              'op_share_of_four_launch_chunk': round(ms['op'][0] / ms['chunk'][0], 4),
              'speedup_vs_torch_fp32': round(ms['torch'][0] / ms['op'][0], 2),
              'note': 'untrained mapping networks: the rows land where their initialisation puts them, not where a trained atlas '
                      'would; hipEvent medians, variants rotated within every repetition'}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
