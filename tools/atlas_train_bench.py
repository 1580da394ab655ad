"""Time one FULL atlas training step (train_atlas.py:127-253) on the GPU at the reference's size: 10 000 sampled pixels,
the widths of the reference's atlas configs, all four networks under one Adam, with and without the two global-rigidity
row blocks.

    python tools/atlas_train_bench.py [--reps 30] [--out profiles/atlas_train_first.json]

Three ways on the same GPU in one process, the order rotated from repetition to repetition:
  fused        ops.atlas_batch (K18a), each network ONCE on its stacked rows, ops.atlas_losses (K18b): atlas_fit.training_losses
  blockwise    the project's own network kernels, called block by block as the reference calls its networks (up to seven calls
               per mapping network), with the CPU fancy-index gathers, the torch.where compactions and the torch loss glue
               of tests/atlas_train_case.py
  torch_fp32   the same block-by-block step with nn.Linear chains and a gathered grid table in place of the kernels
Also: K18a and K18b alone, and the step's kernel-launch count each way (torch.profiler's device events of one step).
The samples are drawn once, outside the timed region (the fused way still copies its 8 N bytes of indices per step; the
other two still gather on the CPU per step, as the reference does).  Times are hipEvent medians after a warm-up; the shader
clock is sampled where the box exposes it.  A first reading with no threshold.  Prints ONE JSON line.
"""
import argparse
import copy
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests'), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

from atlas_bench import TorchChain, median_ms  # noqa: E402
from hash_fit_bench import MODELS, PIXELS, TorchHashChain  # noqa: E402

W, H, T = 256, 256, 8


def launches_of(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if str(e.device_type).endswith('CUDA') and 'Memcpy' not in e.name and 'Memset' not in e.name)
    except Exception as e:  # pragma: no cover
        return f'not counted: {e}'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('atlas_train_bench needs the GPU: nothing here can be timed on the CPU')
    import atlas_train_case as tc
    from videoswap_amd import atlas, atlas_fit, ops
    from videoswap_amd.telemetry import BoardPower
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.manual_seed(0)
    ours = {k: atlas.build_network(kw).cuda().differentiable_(True) for k, kw in MODELS.items()}
    with torch.no_grad():
        ours['F_Atlas'].encoder.params.uniform_(-0.1, 0.1)
    theirs = {k: (TorchHashChain(copy.deepcopy(m)) if k == 'F_Atlas' else TorchChain(copy.deepcopy(m).differentiable_(False)))
              for k, m in ours.items()}
    data = tc.synthetic_data(W, H, T, seed=0)
    on_gpu = atlas_fit.data_to_device(data, 'cuda')
    idx = torch.randint(T * H * W, (PIXELS, 1))
    train = dict(atlas_fit.TRAIN_OPT)
    result = {'metric': 'atlas_training_step', 'device': torch.cuda.get_device_name(0), 'pixels': PIXELS, 'video': [W, H, T], 'reps': args.reps}

    class OnDevice(tc.NetEval):
        def __call__(self, name, x, block, sel=None, layer=None):
            return self.nets[name](x.to(device='cuda', dtype=torch.float32))

    def ways(step):
        with_global = step <= train['pretrain_global_rigidity_iter']

        def fused(models, opt):
            def run():
                b = ops.atlas_batch(idx, on_gpu, train['derivative_amount'], train['global_derivative_amount'], with_global_rigidity=with_global)
                loss, _ = atlas_fit.training_losses(models, b, train, step)
                opt.zero_grad()
                loss.backward()
                opt.step()
            return run

        def blockwise(models, opt):
            def run():
                q = tc.Queries.from_data(tc.jif_of(idx, H, W), data, train['derivative_amount'], train['global_derivative_amount']).to('cuda')
                loss, _ = tc.step_restated(OnDevice(models, torch.float32), q, train, True, with_global, torch.float32)
                opt.zero_grad()
                loss.backward()
                opt.step()
            return run
        out = {}
        for name, make, models in (('fused', fused, ours), ('blockwise', blockwise, ours), ('torch_fp32', blockwise, theirs)):
            out[name] = make(models, torch.optim.Adam([q for m in models.values() for q in m.parameters()], lr=1e-4))
        return out

    with BoardPower() as power:
        for tag, step in (('with_global_rigidity', 0), ('without_global_rigidity', train['pretrain_global_rigidity_iter'] + 1)):
            fns = ways(step)
            names = list(fns)
            for fn in fns.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            times = {k: [] for k in names}
            for rep in range(args.reps):
                for k in names[rep % 3:] + names[:rep % 3]:            # the order rotates
                    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                    ev[0].record()
                    fns[k]()
                    ev[1].record()
                    ev[1].synchronize()
                    times[k].append(ev[0].elapsed_time(ev[1]))
            result[tag] = {k: {'step_ms': round(statistics.median(v), 4), 'step_ms_min_max': [round(min(v), 4), round(max(v), 4)],
                               'kernel_launches': launches_of(fns[k])} for k, v in times.items()}
        b = ops.atlas_batch(idx, on_gpu, 1, 100)
        dev_idx = idx.cuda()
        outs = [torch.rand(9 * PIXELS, 2, device='cuda') * 2 - 1, torch.rand(9 * PIXELS, 2, device='cuda') * 2 - 1,
                torch.rand(5 * PIXELS, device='cuda') * 1.9 - 0.95, torch.rand(6 * PIXELS, 3, device='cuda') * 2 - 1]
        cfg = atlas_fit.loss_kernel_cfg(train, 0)
        for name, fn in (('atlas_batch_with_index_copy', lambda: ops.atlas_batch(idx, on_gpu, 1, 100)),
                         ('atlas_batch_index_on_device', lambda: ops.atlas_batch(dev_idx, on_gpu, 1, 100)),
                         ('atlas_losses', lambda: ops.atlas_losses(*outs, b, cfg))):
            med, lo, hi = median_ms(fn, args.reps)
            result.setdefault('kernels_alone_ms', {})[name] = [round(med, 4), round(lo, 4), round(hi, 4)]
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
