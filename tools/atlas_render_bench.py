"""Time the hash-grid texture network (ops.hash_mlp, ops.hash_grid: csrc/atlas.hip K14) and the rendering of an atlas
(atlas.render_atlas) at the sizes of the reference's configs: F_Atlas 2 -> hash grid (16 levels x 2 features, 2^19
entries) -> 8 layers of 256 with skips [4, 7] -> 3; the mapping networks hidden 256, 6 layers; F_Alpha hidden 256, 8
layers, sin/cos encoding with 5 frequencies.  Weights at the nn.Linear default initialisation, the table uniform in
[-1e-4, 1e-4].

    python tools/atlas_render_bench.py [--reps 10] [--out profiles/atlas_render_bench.json]

F_Atlas: every pixel of a 768 x 448 frame (344 064 rows, uniform in [0, 1]^2) in one launch.  Rendering: one frame and
72 frames through atlas.render_atlas.  Each figure stands beside the same computation as fp32 PyTorch-ROCm on the same
GPU: a torch gather restatement of the grid plus a chain of nn.Linear.  The share of the encoding stage is the time of
`hash_grid` ALONE (its gathers and its [N, 32] store) over the fused launch: the fused kernel is not instrumented.
Times are hipEvent medians after a warm-up of the same shapes; the FLOP are 2 * rows * sum(in * out) over the layers
(unpadded, the interpolation not counted), the fraction is of the 157.3 TF/s fp32 matrix peak; the shader clock is
sampled from sysfs where the box exposes it.  Prints ONE JSON line.
"""
import argparse
import json
import os
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from atlas_bench import PEAK_FP32_MATRIX, TorchChain, flop_per_row, median_ms  # noqa: E402

RES_X, RES_Y, FRAMES = 768, 448, 72
MAPPING = dict(input_dim=3, output_dim=2, hidden_dim=256, pe_type='none', pe_dim=4, mlp_layers=6, skip_layers=[])
MODELS = {
    'FG_UV_Mapping': MAPPING, 'BG_UV_Mapping': MAPPING, 'FG_UV_Mapping_Inverse': dict(MAPPING, output_dim=3),
    'F_Alpha': dict(input_dim=3, output_dim=1, hidden_dim=256, pe_type='encoding', pe_dim=5, mlp_layers=8, skip_layers=[]),
    'F_Atlas': dict(input_dim=2, output_dim=3, hidden_dim=256, pe_type='hash_encoding', pe_dim=10, mlp_layers=8, skip_layers=[4, 7]),
}


class TorchHashChain(nn.Module):
    """the grid of include/vsx.h K14 as torch gathers (int64 arithmetic masked to 32 bits), then the nn.Linear chain"""

    def __init__(self, mlp):
        super().__init__()
        from videoswap_amd.atlas import hash_grid_levels
        self.mlp, self.levels = mlp, hash_grid_levels(mlp.grid)

    def encode(self, x):
        M = 0xffffffff
        tab = self.mlp.encoder.params.view(-1, 2)
        cols = []
        for lv in self.levels:
            pos = lv['scale'] * x + 0.5
            cell = torch.floor(pos)
            w = pos - cell
            g = cell.to(torch.int64) & M
            acc = 0
            for c in range(4):
                c0, c1 = (g[:, 0] + (c & 1)) & M, (g[:, 1] + (c >> 1)) & M
                idx = (c0 ^ ((c1 * 2654435761) & M)) if lv['hashed'] else ((c0 + c1 * lv['res']) & M)
                idx = idx % lv['entries'] + lv['offset']
                weight = (w[:, 0] if c & 1 else 1 - w[:, 0]) * (w[:, 1] if c >> 1 else 1 - w[:, 1])
                acc = acc + weight.unsqueeze(1) * tab[idx]
            cols.append(acc)
        return torch.cat(cols, dim=1)

    def forward(self, x):
        m = self.mlp
        x = self.encode(x)
        inp = x
        for i, layer in enumerate(m.hidden):
            if i > 0:
                x = F.relu(x)
            if i in m.skip_layers:
                x = torch.cat((x, inp), 1)
            x = layer(x)
        return torch.tanh(x) if m.use_tanh else x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('atlas_render_bench needs the GPU: nothing here can be timed on the CPU')
    from videoswap_amd import atlas, ops
    from videoswap_amd.telemetry import BoardPower
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.manual_seed(0)
    nets = {n: atlas.build_network(kw).cuda() for n, kw in MODELS.items()}
    chains = {n: (TorchHashChain(m) if isinstance(m, atlas.HashGridMLP) else TorchChain(m)) for n, m in nets.items()}
    fa, fa_chain = nets['F_Atlas'], chains['F_Atlas']
    N = RES_X * RES_Y
    uv = torch.rand(N, 2, device='cuda').contiguous()
    table = fa.encoder.params.detach()
    result = {'metric': 'atlas_render', 'device': torch.cuda.get_device_name(0), 'rows_per_frame': N, 'reps': args.reps,
              'peak_fp32_matrix_tflops': PEAK_FP32_MATRIX / 1e12, 'grid': fa.grid, 'table_MB': round(table.numel() * 4 / 1e6, 2)}
    with torch.no_grad(), BoardPower() as power:
        diff = float((fa(uv[:4096]) - fa_chain(uv[:4096])).abs().max())
        k_ms, k_lo, k_hi = median_ms(lambda: fa(uv), args.reps)
        g_ms, g_lo, g_hi = median_ms(lambda: ops.hash_grid(uv, table, fa.grid), args.reps)
        t_ms, t_lo, t_hi = median_ms(lambda: fa_chain(uv), max(3, args.reps // 2))
        te_ms, _, _ = median_ms(lambda: fa_chain.encode(uv), max(3, args.reps // 2))
        flop = flop_per_row(fa) * N
        result['F_Atlas_one_frame'] = {
            'kernel_ms': round(k_ms, 4), 'kernel_ms_min_max': [round(k_lo, 4), round(k_hi, 4)],
            'hash_grid_alone_ms': round(g_ms, 4), 'hash_grid_alone_ms_min_max': [round(g_lo, 4), round(g_hi, 4)],
            'encoding_share_of_fused_launch': round(g_ms / k_ms, 4),
            'torch_fp32_ms': round(t_ms, 4), 'torch_fp32_ms_min_max': [round(t_lo, 4), round(t_hi, 4)],
            'torch_fp32_encoding_ms': round(te_ms, 4), 'speedup_vs_torch_fp32': round(t_ms / k_ms, 3),
            'gflop': round(flop / 1e9, 2), 'kernel_tflops': round(flop / k_ms / 1e9, 2),
            'fraction_of_fp32_matrix_peak': round(flop / (k_ms * 1e-3) / PEAK_FP32_MATRIX, 4),
            'ns_per_row': round(k_ms * 1e6 / N, 3), 'max_abs_diff_kernel_vs_torch_4096_rows': diff}
        clocks = power.summary(skip_frac=0.25)
        result['sclk_MHz_mean_min'] = [clocks.get('sclk_mean_MHz'), clocks.get('sclk_min_MHz')] if clocks else 'not exposed by this box'

        render_flop = N * (flop_per_row(nets['FG_UV_Mapping']) + flop_per_row(nets['BG_UV_Mapping']) + flop_per_row(nets['F_Alpha'])
                           + 2 * flop_per_row(fa))
        for label, frames, reps in (('render_1_frame', [0], args.reps), ('render_72_frames', None, max(2, args.reps // 5))):
            n = 1 if frames else FRAMES
            rk, rk_lo, rk_hi = median_ms(lambda: atlas.render_atlas(nets, RES_X, RES_Y, FRAMES, frames=frames), reps, warmup=1)
            rt, rt_lo, rt_hi = median_ms(lambda: atlas.render_atlas(chains, RES_X, RES_Y, FRAMES, frames=frames),
                                         max(2, reps // 2), warmup=1)
            result[label] = {'kernel_ms': round(rk, 3), 'kernel_ms_min_max': [round(rk_lo, 3), round(rk_hi, 3)],
                             'torch_fp32_ms': round(rt, 3), 'torch_fp32_ms_min_max': [round(rt_lo, 3), round(rt_hi, 3)],
                             'speedup_vs_torch_fp32': round(rt / rk, 3), 'ms_per_frame': round(rk / n, 3),
                             'network_tflops': round(render_flop * n / rk / 1e9, 2),
                             'note': 'four network launches per 2^20-row chunk plus the torch glue (coordinates, blend)'}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
