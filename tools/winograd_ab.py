"""A/B of the two forms of the stride-1 3x3 convolutions at the UNet's real shapes: the direct implicit-GEMM kernels
(option conv_winograd = 0) against Winograd F(2x2, 3x3) (conv_winograd = 2: input transform + batched GEMM + output
transform, csrc/winograd.hip).

    python tools/winograd_ab.py [--batches 1,2] [--rounds 7] > profiles/winograd_ab.txt

Method of tools/gemm_ab.py: the variants are interleaved round by round inside ONE process, the order rotating; the table
shows the median of the per-round times and each variant's spread (min .. max over the rounds).  `gemm` is the batched GEMM
stage alone on buffers of the same sizes, `xform` = winograd - gemm (the two transform kernels together; a kernel-stats
profile splits them).  A shape is a gain where the Winograd maximum lies below the direct minimum."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from videoswap_amd import ops  # noqa: E402
from videoswap_amd._lib import GemmDesc  # noqa: E402
from gemm_ab import r, shapes, time_once  # noqa: E402


def make_conv(a, residual):
    hw, cin = a['hw'], a['c1'] + a['c2']
    x = r(a['nimg'], hw, hw, a['c1'])
    x2 = r(a['nimg'], hw, hw, a['c2']) if a['c2'] else None
    w, b = r(a['co'], 3, 3, cin, scale=(9 * cin) ** -0.5), r(a['co'])
    rv = None if residual else r(a['nimg'] // 16, a['co'])
    res = r(a['nimg'], hw, hw, a['co']) if residual else None
    return lambda: ops.conv2d(x, w, b, x2=x2, rowvec=rv, rows_per_vec=16 * hw * hw, residual=res)


def make_gemm_stage(a):
    tiles, cin, co = a['nimg'] * a['hw'] * a['hw'] // 4, a['c1'] + a['c2'], a['co']
    v, u = r(16, tiles, cin), r(16, co, cin, scale=cin ** -0.5)
    out = torch.empty(16, tiles, co, dtype=torch.float16, device='cuda')
    d = GemmDesc()
    d.M, d.N, d.K = tiles, co, cin
    d.batch0, d.batch1 = 16, 1
    d.A = v.data_ptr(); d.lda = cin; d.a_bs0 = tiles * cin
    d.B = u.data_ptr(); d.ldb = cin; d.b_bs0 = co * cin
    d.C = out.data_ptr(); d.ldc = co; d.c_bs0 = tiles * co
    d.alpha = 1.0
    keep = (v, u, out)
    return lambda: (ops.gemm(d), keep)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='1,2')
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--reps', type=int, default=4)
    ap.add_argument('--levels', default='8,16,32,64')
    args = ap.parse_args()
    levels = [int(x) for x in args.levels.split(',')]
    print(f'# T=16 64x64 latent; median (min .. max) of {args.rounds} rotated rounds x {args.reps} launches; times in us')
    print(f'{"shape":46s} {"n":>3s} {"direct":>24s} {"winograd":>24s} {"gemm":>8s} {"xform":>7s}  {"change":>7s}  verdict')
    for B in (int(x) for x in args.batches.split(',')):
        tot_d = tot_w = tot_gain = 0.0
        for kind, name, a, count in shapes(B):
            if kind != 'conv' or a['stride'] != 1 or a['up'] or a['hw'] not in levels:
                continue
            forms = [(False, count)]
            if a['c2'] == 0 and a['c1'] == a['co']:      # a resnet's conv2 carries the residual: half of the C -> C launches
                forms = [(False, count - count // 2), (True, count // 2)]
            for residual, n in forms:
                if n == 0:
                    continue
                torch.manual_seed(0)
                fn, gemm = make_conv(a, residual), make_gemm_stage(a)
                variants = [('direct', 0, fn), ('winograd', 2, fn), ('gemm', 0, gemm)]
                ts = {v[0]: [] for v in variants}
                for v in variants:
                    ops.set_option('conv_winograd', v[1])
                    v[2]()
                torch.cuda.synchronize()
                for rnd in range(args.rounds):
                    k = rnd % len(variants)
                    for v in variants[k:] + variants[:k]:
                        ops.set_option('conv_winograd', v[1])
                        ts[v[0]].append(time_once(v[2], args.reps) * 1000.0)
                med = {k: sorted(x)[len(x) // 2] for k, x in ts.items()}
                d, w = ts['direct'], ts['winograd']
                verdict = 'gain' if max(w) < min(d) else ('loss' if min(w) > max(d) else 'inside the spread')
                tot_d += med['direct'] * n / 1000.0
                tot_w += med['winograd'] * n / 1000.0
                if verdict == 'gain':
                    tot_gain += (med['direct'] - med['winograd']) * n / 1000.0
                label = f'B={B} {name}' + (' +res' if residual else ' +rowvec')
                print(f'{label:46s} {n:3d} {med["direct"]:8.1f} ({min(d):6.1f} ..{max(d):7.1f}) {med["winograd"]:8.1f} ({min(w):6.1f} ..{max(w):7.1f}) '
                      f'{med["gemm"]:8.1f} {med["winograd"] - med["gemm"]:7.1f}  {100.0 * (med["winograd"] / med["direct"] - 1.0):+6.1f}%  {verdict}',
                      flush=True)
        print(f'# B={B}: listed launches per forward: direct {tot_d:.2f} ms, winograd everywhere {tot_w:.2f} ms, '
              f'taking the gains only saves {tot_gain:.2f} ms')
    ops.set_option('conv_winograd', 1)


if __name__ == '__main__':
    main()
