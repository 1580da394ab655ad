"""Time one step of atlas.pretrain_mapping on the GPU: the FG_UV_Mapping network of 4022_4_atlas_rabbit_inv_fp32.yml
(3 -> 2, hidden 256, 6 layers, pe none), N = 10 000 rows: training forward (ops.coord_mlp_train_forward), the loss in
torch, backward (ops.coord_mlp_backward, csrc/atlas_bwd.hip), one Adam step.

    python tools/atlas_fit_bench.py [--reps 20] [--out profiles/atlas_fit_first.json]

The comparison line is the same network as a chain of nn.Linear in fp32 under PyTorch-ROCm autograd on the same GPU, same
loss, same optimizer.  The samples are drawn once, outside the timed region (the reference draws them on the CPU; that cost
is the same for both).  Times are hipEvent medians after a warm-up of the same shapes, as tools/atlas_bench.py measures;
forward + backward alone (no loss, no optimizer: the cotangent is fixed) is timed as well.  A first reading with no
threshold.  Prints ONE JSON line.
"""
import argparse
import copy
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from atlas_bench import TorchChain, flop_per_row, median_ms  # noqa: E402

SPEC = dict(input_dim=3, output_dim=2, hidden_dim=256, pe_type='none', pe_dim=4, mlp_layers=6, skip_layers=[])
N, SCALE = 10000, 0.9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('atlas_fit_bench needs the GPU: nothing here can be timed on the CPU')
    from videoswap_amd import atlas
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.manual_seed(0)
    ours = atlas.CoordMLP(**SPEC).cuda().differentiable_(True)
    chain = TorchChain(copy.deepcopy(ours).differentiable_(False))
    xyt = (torch.rand(N, 3, device='cuda') * 2 - 1).contiguous()
    G = torch.randn(N, 2, device='cuda') / N

    def step_fn(model, params):
        opt = torch.optim.Adam(params, lr=1e-4)

        def step():
            uv = model(xyt)
            opt.zero_grad()
            loss = (xyt[:, :2] * SCALE - uv).norm(dim=1).mean()
            loss.backward()
            opt.step()
        return step

    def fwd_bwd_fn(model, params):
        def run():
            for q in params:
                q.grad = None
            (model(xyt) * G).sum().backward()
        return run

    res = {}
    for name, model, params in (('kernel', ours, list(ours.parameters())), ('torch_fp32', chain, list(chain.mlp.parameters()))):
        fb, fb_lo, fb_hi = median_ms(fwd_bwd_fn(model, params), args.reps)
        st, st_lo, st_hi = median_ms(step_fn(model, params), args.reps)
        res[name] = {'forward_backward_ms': round(fb, 4), 'forward_backward_ms_min_max': [round(fb_lo, 4), round(fb_hi, 4)],
                     'step_ms': round(st, 4), 'step_ms_min_max': [round(st_lo, 4), round(st_hi, 4)], 'steps_per_second': round(1e3 / st, 1)}
    flop = 3 * flop_per_row(ours) * N            # forward, data gradient, weight gradient (layer 0 has no data gradient: slightly less)
    result = {'metric': 'atlas_fit_pretrain_step', 'device': torch.cuda.get_device_name(0), 'rows': N, 'network': SPEC, 'reps': args.reps,
              'gflop_forward_backward_nominal': round(flop / 1e9, 2), **res,
              'kernel_forward_backward_tflops_nominal': round(flop / res['kernel']['forward_backward_ms'] / 1e9, 2),
              'kernel_steps_per_second_vs_torch_fp32': round(res['torch_fp32']['step_ms'] / res['kernel']['step_ms'], 3)}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
