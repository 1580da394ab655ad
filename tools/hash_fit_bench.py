"""Time one step of atlas.fit_reconstruction on the GPU at the reference's size: 10 000 pixels (20 000 F_Atlas rows), the
widths of the reference's atlas configs (mappings 256 x 6 / 256 x 4, F_Alpha 256 x 8 behind the sin/cos encoding, F_Atlas
256 x 8 with skips [4, 7] behind the reference's HASH_GRID), all four networks trained by one Adam.

    python tools/hash_fit_bench.py [--reps 30] [--out profiles/hash_fit_first.json]

Parts of F_Atlas's share at 20 000 rows, each timed alone: the training forward (ops.hash_mlp_train_forward), the backward
without a grid gradient (the K16 chain: ops.hash_mlp_backward with neither table nor x wanted), the whole backward, and the
grid backward alone (ops.hash_grid_backward) with the table only, with x only and with both; dEnc is the whole backward
minus the chain minus the grid backward (derived, not timed).  grid_backward_share = grid backward (both) / whole backward
decides whether the dense levels are pre-summed in LDS.

The comparison line is the same step as an fp32 torch restatement on the same GPU: the grid as gathers of a table
parameter (its gradient is autograd's index_put with accumulate), nn.Linear chains, the same losses and optimizer.  The
samples are drawn once, outside the timed region.  Times are hipEvent medians after a warm-up of the same shapes; the shader
clock is sampled during the run where the box exposes it.  A first reading with no threshold.  Prints ONE JSON line.
"""
import argparse
import copy
import json
import os
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from atlas_bench import TorchChain, median_ms  # noqa: E402

PIXELS = 10000
MAPPING = dict(input_dim=3, output_dim=2, hidden_dim=256, pe_type='none', pe_dim=4, mlp_type='origin', mlp_layers=6, skip_layers=[],
               use_tanh=True, fp16=False)
MODELS = {'FG_UV_Mapping': dict(MAPPING), 'BG_UV_Mapping': dict(MAPPING, mlp_layers=4),
          'F_Alpha': dict(MAPPING, output_dim=1, pe_type='encoding', pe_dim=5, mlp_layers=8),
          'F_Atlas': dict(input_dim=2, output_dim=3, hidden_dim=256, pe_type='hash_encoding', pe_dim=10, mlp_type='origin',
                          mlp_layers=8, skip_layers=[4, 7], use_tanh=True, fp16=False)}


class TorchHashChain(nn.Module):
    """HashGridMLP as PyTorch runs it: per level four gathers of the table parameter, then the nn.Linear chain"""

    def __init__(self, net):
        super().__init__()
        from videoswap_amd.atlas import hash_grid_levels
        self.net, self.levels = net, hash_grid_levels(net.grid)
        self.table = nn.Parameter(net.encoder.params.detach().clone().view(-1, 2))

    def forward(self, x):
        cols = []
        for lv in self.levels:
            pos = lv['scale'] * x + 0.5
            cell = torch.floor(pos.detach())
            w = pos - cell
            g = cell.to(torch.int64) & 0xffffffff
            acc = 0
            for c in range(4):
                c0, c1 = (g[:, 0] + (c & 1)) & 0xffffffff, (g[:, 1] + (c >> 1)) & 0xffffffff
                idx = c0 ^ ((c1 * 2654435761) & 0xffffffff) if lv['hashed'] else (c0 + c1 * lv['res']) & 0xffffffff
                weight = (w[:, 0] if c & 1 else 1 - w[:, 0]) * (w[:, 1] if c >> 1 else 1 - w[:, 1])
                acc = acc + weight.unsqueeze(1) * self.table[idx % lv['entries'] + lv['offset']]
            cols.append(acc)
        h = torch.cat(cols, dim=1)
        inp = h.detach().clone()
        for i, layer in enumerate(self.net.hidden):
            if i > 0:
                h = F.relu(h)
            if i in self.net.skip_layers:
                h = torch.cat((h, inp), 1)
            h = layer(h)
        return torch.tanh(h) if self.net.use_tanh else h

    def parameters(self, recurse=True):
        return [self.table] + list(self.net.hidden.parameters())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('hash_fit_bench needs the GPU: nothing here can be timed on the CPU')
    from videoswap_amd import atlas, ops
    from videoswap_amd.telemetry import BoardPower
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.manual_seed(0)
    ours = {k: atlas.build_network(kw).cuda().differentiable_(True) for k, kw in MODELS.items()}
    with torch.no_grad():
        ours['F_Atlas'].encoder.params.uniform_(-0.1, 0.1)           # a texture that is not flat: the gradients are not denormal
    theirs = {k: (TorchHashChain(copy.deepcopy(m)) if k == 'F_Atlas' else TorchChain(copy.deepcopy(m).differentiable_(False)))
              for k, m in ours.items()}
    xyt = (torch.rand(PIXELS, 3, device='cuda') * 2 - 1).contiguous()
    rgb, alpha_gt = torch.rand(PIXELS, 3, device='cuda'), (torch.rand(PIXELS, 1, device='cuda') > 0.5).float()

    def step_fn(models, params):
        opt = torch.optim.Adam(params, lr=1e-4)

        def step():
            loss, _ = atlas.reconstruction_losses(models, xyt, rgb, alpha_gt, None, True)
            opt.zero_grad()
            loss.backward()
            opt.step()
        return step

    result = {'metric': 'hash_fit_reconstruction_step', 'device': torch.cuda.get_device_name(0), 'pixels': PIXELS, 'atlas_rows': 2 * PIXELS,
              'grid': atlas.HASH_GRID, 'reps': args.reps}
    with BoardPower() as power:
        for name, models in (('kernel', ours), ('torch_fp32', theirs)):
            params = [q for m in models.values() for q in m.parameters()]
            st, lo, hi = median_ms(step_fn(models, params), args.reps)
            result[name] = {'step_ms': round(st, 4), 'step_ms_min_max': [round(lo, 4), round(hi, 4)], 'steps_per_second': round(1e3 / st, 1)}

        # F_Atlas's parts at 2 * PIXELS rows
        net = ours['F_Atlas']
        kw = dict(output_dim=net.output_dim, hidden_dim=net.hidden_dim, mlp_layers=net.mlp_layers, skip_layers=net.skip_layers,
                  use_tanh=net.use_tanh)
        N, E = 2 * PIXELS, net.encoding_dimensions
        x = torch.rand(N, 2, device='cuda') * 2 - 1
        table, packed = net.encoder.params.detach(), net.packed()
        out, saved = ops.hash_mlp_train_forward(x, table, net.grid, packed, **kw)
        gout, genc = torch.randn(N, 3, device='cuda') / N, torch.randn(N, E, device='cuda') / N
        parts = {
            'train_forward': lambda: ops.hash_mlp_train_forward(x, table, net.grid, packed, **kw, saved=saved),
            'plain_forward': lambda: ops.hash_mlp(x, table, net.grid, packed, **kw),
            'backward_layers_only': lambda: ops.hash_mlp_backward(gout, x, table, net.grid, saved, packed, **kw, want_table=False, want_x=False),
            'backward_all': lambda: ops.hash_mlp_backward(gout, x, table, net.grid, saved, packed, **kw),
            'grid_backward_table_only': lambda: ops.hash_grid_backward(x, genc, table, net.grid, want_x=False),
            'grid_backward_x_only': lambda: ops.hash_grid_backward(x, genc, table, net.grid, want_table=False),
            'grid_backward_both': lambda: ops.hash_grid_backward(x, genc, table, net.grid),
            'clear_table_gradient': lambda: torch.zeros_like(table),
        }
        ms = {}
        for k, fn in parts.items():
            med, lo, hi = median_ms(fn, args.reps)
            ms[k] = med
            result.setdefault('f_atlas_parts_ms', {})[k] = [round(med, 4), round(lo, 4), round(hi, 4)]
    result['f_atlas_parts_ms']['denc_derived'] = round(ms['backward_all'] - ms['backward_layers_only'] - ms['grid_backward_both'], 4)
    result['grid_backward_share_of_backward'] = round(ms['grid_backward_both'] / ms['backward_all'], 4)
    result['table_adds_per_call'] = N * int(net.grid['n_levels']) * 8
    result['kernel_steps_per_second_vs_torch_fp32'] = round(result['torch_fp32']['step_ms'] / result['kernel']['step_ms'], 3)
    clocks = power.summary(skip_frac=0.25)
    result['sclk_MHz_mean_min'] = [clocks.get('sclk_mean_MHz'), clocks.get('sclk_min_MHz')] if clocks else 'not exposed by this box'
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
