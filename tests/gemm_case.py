"""Shared by tests/test_gemm_kernels_gpu.py (the HIP kernels of videoswap_amd/csrc/gemm.hip and gemm_pp.hip behind vsx_gemm_f16) and
tests/test_gemm_case.py (a CPU restatement of the descriptor, and deliberate mutants of it): the case tables, the input makers, fp64
references written on the DESCRIPTOR (every field of vsx_gemm_desc the tables use), the rule and the runners.  No kernels and no GPU
calls of its own: every runner takes `impl` (what launches a descriptor) and a device.

Two input classes.

  E (exact)    A, B integers in [-3, 3]; bias EVEN integers with 2048 <= |b| <= 4094; row vector and residual integers in [-2047,
               2047]; alpha in {1, 0.25, 2}; the folded LayerNorm through the raw fields, rowscale = (2^j, integer), colvec = integers.
               Every value is fp16-exact and every partial sum stays below 2^24, so EVERY summation order gives the same fp32 number:
               the only correct output is the exact value rounded to fp16 ONCE.  The rule: the stored bits equal the fp64 reference
               rounded to fp16.  No tolerance, no case left out.  The bias range puts acc + bias beyond 2048, where fp16 steps by 2 and
               every odd sum is a tie: a second rounding (before the residual, a bias added in fp16) shows in a quarter of the
               elements, and one element that lost one 8-wide K tail shows as exactly that element.  Row-statistics cases keep
               |out| <= 64 (`small`): the (sum, sum of squares) parts are then exact as well.
  R (rounded)  Gaussian fp16 inputs, for what is not exact: GEGLU, the fold with a real rstd, a residual 64 x the product.  want = the
               chain in fp64; ideal = the documented chain in fp32 (alpha, fold, bias, GEGLU in the erf form, row vector, residual
               last) rounded once.  train_kernel_case.measure unchanged, with the per-element extra
                   2^-10 rms(row) + (K + 4) 2^-24 S,   S = sum_k |a||b| + |bias| + |rowvec| + |residual|
               (the worst case of any fp32 summation order of those terms), for GEGLU propagated through h * gelu(g) to first order,
               plus train_kernel_case's erf-form term 1e-5 |h| max(1, |g|).

Guard bands, in every case of both classes: C sits inside a buffer prefilled with a sentinel, with rows in front and behind and
ldc = N + pad, pad in {0, 1, 4, 8} (the scalar, 8-byte and 16-byte stores); the residual has its own ldr != ldc; the transposed store
has ldvt > rows and a gap between images.  After the launch every element outside the result is bit-identical to before.  A and B
have lda = ldb = K + 8 with the eight pad columns set to 60000: an unmasked K tail overflows instead of cancelling.

Every case names the plan (vsx_gemm_plan) it is aimed at, and the runner asserts it before it launches: a case that the planner
sends elsewhere fails instead of passing on another kernel.
"""
import contextlib
import ctypes
import math

import torch
import torch.nn.functional as F

import train_kernel_case as tk
from train_kernel_case import H, measure

BK = 64
PAD_VALUE = 60000.0
SENTINEL = -1234.0
FIGURES = []                    # one dict per case run
WS, PP256, PP128, TILE = 0, 1, 2, 3
# every option a case may depend on, with the value the tables start from (NOT the library's defaults: those are saved and restored)
BASE_OPTS = dict(gemm_pp=0, gemm_ws=0, ws_waves=10, tile_tune=0, pp_sched=0, xcd_walk=1, conv_winograd=0)
FORCED_TILE = {1: (128, 320), 2: (128, 160), 3: (256, 320), 4: (128, 128), 5: (64, 128), 6: (64, 64)}
RING = {(64, 64): 4, (64, 128): 4, (128, 128): 2, (128, 160): 2, (128, 320): 2, (256, 320): 2}      # launch_tile: NST
RPAD = {0: 8, 1: 2, 4: 12, 8: 16}       # ldr = N + RPAD[pad]: never ldc, and 8- / 16-byte aligned exactly where ldc is
RULE = ('E: stored bits == the fp64 reference rounded to fp16 once, guards untouched.  R: train_kernel_case.measure (l2 <= 1.5 ideal, '
        'worst row <= 2 ideal, max-abs <= 4 ideal, per element <= 1 fp16 ulp + extra), ideal = the documented chain in fp32 rounded '
        'once, extra = 2^-10 rms(row) + (K + 4) 2^-24 S, S = sum |a||b| + |bias| + |rowvec| + |residual| (GEGLU: first-order through '
        'h gelu(g), + 1e-5 |h| max(1, |g|)); guards untouched')


def round_up(x, m):
    return (x + m - 1) // m * m


# ------------------------------------------------------------------------------------------------
# what the runners need from `impl` beyond the launch: the library's host-side queries (no HIP call in any of them)
# ------------------------------------------------------------------------------------------------
class LibQueries:
    """plan / workspace / check / options through videoswap_amd._lib.  A subclass adds gemm(desc), sync() and the wrappers."""

    def __init__(self):
        from videoswap_amd import _lib
        self._lib = _lib
        self.GemmDesc = _lib.GemmDesc

    def lib(self):
        return self._lib.load()

    def plan(self, d):
        out = (ctypes.c_int64 * 8)()
        rc = self.lib().vsx_gemm_plan(ctypes.byref(d), out)
        return rc, dict(zip(('family', 'BM', 'BN', 'deep', 'splits', 'nk_per', 'stat_parts', 'refused'), (int(v) for v in out)))

    def workspace(self, d):
        return int(self.lib().vsx_gemm_workspace(ctypes.byref(d)))

    def rowstats_parts(self, d):
        return int(self.lib().vsx_gemm_rowstats_parts(ctypes.byref(d)))

    def check(self, d):
        return int(self.lib().vsx_gemm_check(ctypes.byref(d)))

    def set_option(self, name, value):
        self._lib.check(self.lib().vsx_set_option(name.encode(), int(value)), 'vsx_set_option')

    def get_option(self, name):
        v = ctypes.c_int64()
        self._lib.check(self.lib().vsx_get_option(name.encode(), ctypes.byref(v)), 'vsx_get_option')
        return v.value

    def sync(self):
        pass


@contextlib.contextmanager
def options(impl, opts):
    """BASE_OPTS overlaid with `opts`; every option is read first and put back, whatever happens in between"""
    want = dict(BASE_OPTS, **opts)
    saved = {k: impl.get_option(k) for k in want}
    try:
        for k, v in want.items():
            impl.set_option(k, v)
        yield
    finally:
        for k, v in saved.items():
            impl.set_option(k, v)


# ------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------
def case(name, M=0, N=0, K=0, epi='', cls='E', pad=0, alpha=1.0, rpv=0, rpi=0, conv=None, batch=None, split=False, align8=False,
         small=False, res_scale=1.0, opts=None, plan=None, status=0):
    """epi: letters b(ias) v(rowvec) r(esidual) g(eglu) f(old) t(ransposed store) s(row statistics).  conv: (nimg, H, W, C1, C2, ks,
    stride, ups, pad_lo, pad_hi) with H x W the SOURCE image (ups: read as its nearest-2x) and pad -1 = symmetric; M, K derived.
    batch: (batch0, batch1, zero): distinct strides, `zero` = B shared by batch0 (b_bs0 = 0).  status: what vsx_gemm_check answers
    (a refusal case is not launched)."""
    c = dict(name=name, M=M, N=N, K=K, epi=epi, cls='R' if 'g' in epi else cls, pad=pad, alpha=alpha, rpv=rpv, rpi=rpi, conv=conv,
             batch=batch, split=split, align8=align8, small=small or 's' in epi, res_scale=res_scale, opts=dict(opts or {}),
             plan=dict(plan or {}), status=status)
    if conv is not None:
        nimg, Hs, Ws, C1, C2, ks, stride, ups, lo, hi = conv
        Hl, Wl = (2 * Hs, 2 * Ws) if ups else (Hs, Ws)
        plo, phi = (ks // 2, ks // 2) if lo < 0 else (lo, hi)
        Ho, Wo = (Hl + plo + phi - ks) // stride + 1, (Wl + plo + phi - ks) // stride + 1
        assert Ho > 0 and Wo > 0, name
        c.update(M=nimg * Ho * Wo, K=ks * ks * (C1 + C2), HoWo=Ho * Wo)
        if rpv == -1:
            c['rpv'] = Ho * Wo
        elif rpv == -2:
            c['rpv'] = 2 * Ho * Wo
    assert 'family' in c['plan'], name
    return c


def case_id(c):
    return c['name']


def _tile_plan(tune):
    bm, bn = FORCED_TILE[tune & 15]
    return dict(family=TILE, BM=bm, BN=bn, deep=1 if (tune & 15) == 2 and (tune & 16) else 0, splits=1)


def _epi_tag(epi, rpv=0, rpi=0):
    return (epi or 'none') + (f'{rpv}' if 'v' in epi and rpv else '') + (f'{rpi}' if 't' in epi else '')


def tile_cases():
    out = []
    # 1. the narrow tiles at every ragged edge: tile_tune 4 / 5 / 6 take any N
    ks, pads, alphas = (8, 56, 64, 72), (0, 1, 4, 8), (1.0, 0.25, 2.0)
    epis = ('', 'b', 'bv', 'br', 'bvr', 'f', 'r', 'bf')
    i = 0
    for tune in (4, 5, 6):
        for M in (1, 63, 64, 65, 129):
            for N in (1, 3, 4, 7, 8, 36, 63, 64, 65, 129, 200):
                epi, K, pad, rpv = epis[i % len(epis)], ks[(i // 2) % 4], pads[(i // 3) % 4], (48, 1, 7)[(i // 8) % 3]
                out.append(case(f'tile{tune}-{M}x{N}x{K}-{_epi_tag(epi, rpv)}-pad{pad}', M, N, K, epi, pad=pad, alpha=alphas[i % 3],
                                rpv=rpv, opts=dict(tile_tune=tune), plan=_tile_plan(tune)))
                i += 1
    # 2. the wide tiles: tile_tune 1 / 2 / 2+16 / 3 need a multiple of 320 rows of B (GEGLU: N = 160)
    epis = ('b', 'br', 'bv', '', 'bvr', 'f', 'fv')
    for tune in (1, 2, 18, 3):
        for N, g in ((320, ''), (640, ''), (160, 'g')):
            for M in (1, 127, 128, 129, 255, 256, 257, 300):
                epi = ('bg', 'bgr', 'g', 'bfg')[i % 4] if g else epis[i % len(epis)]
                K, pad = (8, 64, 72, 136)[i % 4], pads[(i // 2) % 4]
                out.append(case(f'tile{tune}-{M}x{N}x{K}-{_epi_tag(epi, 48)}-pad{pad}', M, N, K, epi, pad=pad,
                                alpha=1.0 if g else alphas[i % 3], rpv=48, opts=dict(tile_tune=tune), plan=_tile_plan(tune)))
                i += 1
    # 3. the K ladder of every instance: 64 n and 64 n + 8 for n = 1 .. ring depth + 2 (the prologue, the steady state and the drain
    #    of the LDS ring each see a full and a ragged last slab)
    for tune, (M, N) in ((6, (65, 72)), (5, (65, 136)), (4, (129, 136)), (2, (129, 320)), (18, (129, 320)), (1, (129, 320)), (3, (257, 320))):
        depth = 4 if tune == 18 else RING[FORCED_TILE[tune & 15]]
        for n in range(1, depth + 3):
            for K in (64 * n, 64 * n + 8):
                out.append(case(f'tile{tune}-ladder-{M}x{N}x{K}', M, N, K, 'br', pad=(0, 8)[n % 2], opts=dict(tile_tune=tune),
                                plan=_tile_plan(tune)))
    # 4. every epilogue on a narrow ragged tile and on a wide one; rows_per_vec 1, a value that splits a tile, and one block
    for tune, (M, N, K) in ((6, (130, 72, 72)), (2, (257, 320, 72))):
        for epi in ('', 'b', 'bv', 'br', 'bvr', 'bg', 'bgr', 'f', 'bf', 'bfg', 'bfv', 'bfr'):
            for rpv in ((1, 48, 130 if tune == 6 else 257) if 'v' in epi else (0,)):
                Nn = N // 2 if 'g' in epi else N
                out.append(case(f'tile{tune}-epi-{M}x{Nn}x{K}-{_epi_tag(epi, rpv)}', M, Nn, K, epi, pad=4 if tune == 6 else 0, rpv=rpv,
                                alpha=1.0 if 'g' in epi else 0.25, opts=dict(tile_tune=tune), plan=_tile_plan(tune)))
    # operands aligned to 8 bytes only (vec4 without the 16-byte forms), and the scalar residual / row vector
    for pad, N in ((0, 72), (4, 72), (1, 70), (0, 70)):
        out.append(case(f'tile6-align8-130x{N}x72-bvr-pad{pad}', 130, N, 72, 'bvr', pad=pad, rpv=48, align8=True, opts=dict(tile_tune=6),
                        plan=_tile_plan(6)))
    out.append(case('tile2-align8-257x320x72-bvr', 257, 320, 72, 'bvr', rpv=48, align8=True, opts=dict(tile_tune=2), plan=_tile_plan(2)))
    # the transposed store: rows per image 77 (scalar), 64 (quads), 5 (an image boundary inside one quad), M past a boundary
    for tune in (6, 2):
        for rpi, nimg in ((77, 2), (64, 3), (5, 27)):
            for epi in ('bt', 'bft', 't'):
                N = 72 if tune == 6 else 320
                out.append(case(f'tile{tune}-vt-{rpi * nimg}x{N}x72-{_epi_tag(epi, rpi=rpi)}', rpi * nimg, N, 72, epi, rpi=rpi,
                                opts=dict(tile_tune=tune), plan=dict(_tile_plan(tune), deep=0)))
    # 5. batch 2 x 3, distinct strides; one zero stride (the weights shared by batch0)
    for tune, (M, N, K) in ((6, (40, 56, 40)), (5, (70, 130, 72)), (2, (130, 320, 72))):
        for zero in (False, True):
            for pad in (0, 1):
                out.append(case(f'tile{tune}-batch2x3-{M}x{N}x{K}-pad{pad}' + ('-sharedB' if zero else ''), M, N, K, 'br', pad=pad,
                                alpha=0.25, batch=(2, 3, zero), opts=dict(tile_tune=tune), plan=_tile_plan(tune)))
    # 6. the XCD block grid against the linear walk at >= 16 tiles: the same bits (both are the exact answer)
    for walk in (0, 1):
        out.append(case(f'tile6-xcd{walk}-256x256x72', 256, 256, 72, 'br', opts=dict(tile_tune=6, xcd_walk=walk), plan=_tile_plan(6)))
        out.append(case(f'tile2-xcd{walk}-1024x640x136', 1024, 640, 136, 'br', opts=dict(tile_tune=2, xcd_walk=walk), plan=_tile_plan(2)))
    # the automatic choice at small shapes (no option forced): the 64 x 64 tile, and the 64 x 128 one under GEGLU
    out.append(case('tile-auto-70x44x72-br-pad1', 70, 44, 72, 'br', pad=1, plan=dict(family=TILE, BM=64, BN=64)))
    out.append(case('tile-auto-90x80x72-bg', 90, 80, 72, 'bg', plan=dict(family=TILE, BM=64, BN=128)))
    return out


def split_cases():
    out = []
    epis = ('', 'b', 'bv', 'br', 'bvr', 'f', 'bfr', 'bfv')
    i = 0
    # nk chosen so that the last slice is shorter than the others: s = 2: 3 slabs (2 + 1); 3: 5 (2 + 2 + 1); 5: 9 (2 x 4 + 1)
    for s, nk in ((2, 3), (3, 5), (5, 9)):
        for M in (1, 100, 129):
            for N in (320, 640):
                K = 64 * nk - (56 if i % 2 else 0)               # (the last, short slice also ends in a K tail every other case)
                epi, pad = epis[i % len(epis)], (0, 4, 8)[i % 3]
                out.append(case(f'split{s}-{M}x{N}x{K}-{_epi_tag(epi, 48)}-pad{pad}', M, N, K, epi, pad=pad, rpv=48, split=True,
                                alpha=(1.0, 0.25, 2.0)[i % 3], opts=dict(tile_tune=256 * s),
                                plan=dict(family=TILE, BM=128, BN=320, splits=s, nk_per=2)))
                i += 1
    # forced counts that would leave the last slice EMPTY (the automatic planner never asks for one): plan_splitk takes slices away
    # until every slice has a slab.  5 slabs in 4 slices: ceil = 2 -> 2 + 2 + 1 + 0, so three slices; 4 in 3 -> two; 7 in 5 -> four
    for s, nk, got in ((4, 5, 3), (3, 4, 2), (5, 7, 4), (8, 3, 3)):
        for M, N in ((100, 320), (129, 640)):
            out.append(case(f'split{s}-empty-last-slice-{M}x{N}x{64 * nk}-br', M, N, 64 * nk, 'br', split=True, opts=dict(tile_tune=256 * s),
                            plan=dict(family=TILE, BM=128, BN=320, splits=got, nk_per=(nk + got - 1) // got)))
    # without a workspace the same descriptor must not split
    out.append(case('split2-no-workspace-100x320x192-br', 100, 320, 192, 'br', opts=dict(tile_tune=512), plan=dict(family=TILE, splits=1)))
    return out


def pp_cases():
    out = []
    epis = ('', 'b', 'r', 'bv', 'f', 'fv', 's', 'rs', 'br', 'bf', 'bs', 'brs')
    i = 0
    for sched in (0, 8):
        for M in (1, 255, 256, 257, 600):
            for N in (320, 640):
                for K in (8, 64, 72, 328):
                    epi = epis[i % len(epis)]
                    parts = N // 320 * 6 if 's' in epi else None
                    plan = dict(family=PP256) if parts is None else dict(family=PP256, stat_parts=parts)
                    out.append(case(f'pp256-sched{sched}-{M}x{N}x{K}-{_epi_tag(epi, 48)}', M, N, K, epi, pad=(0, 8)[i % 2], rpv=48,
                                    alpha=1.0 if 's' in epi else (1.0, 0.25, 2.0)[i % 3], opts=dict(gemm_pp=4, pp_sched=sched), plan=plan))
                    i += 1
    for M in (1, 257, 600):                       # GEGLU (alpha 1), with and without the fold
        for epi in ('bg', 'bfg', 'g'):
            out.append(case(f'pp256-{M}x160x72-{epi}', M, 160, 72, epi, opts=dict(gemm_pp=4), plan=dict(family=PP256)))
            out.append(case(f'pp256-{M}x320x328-{epi}', M, 320, 328, epi, pad=8, opts=dict(gemm_pp=4, pp_sched=8), plan=dict(family=PP256)))
    for epi in ('bt', 'bft', 't'):                # the transposed store: whole 256-row tiles inside one image
        out.append(case(f'pp256-vt-512x320x72-{epi}256', 512, 320, 72, epi, rpi=256, opts=dict(gemm_pp=4), plan=dict(family=PP256)))
        out.append(case(f'pp256-vt-1024x640x64-{epi}512', 1024, 640, 64, epi, rpi=512, opts=dict(gemm_pp=4, pp_sched=8), plan=dict(family=PP256)))
    # more tiles than CUs: 130 x 2 = 260 tiles of 256 rows
    out.append(case('pp256-33280x640x64-br', 33280, 640, 64, 'br', opts=dict(gemm_pp=4), plan=dict(family=PP256)))
    # 128-row tiles from 32 of them
    for sched in (0, 8):
        for epi in ('', 'br', 'bv', 'f', 'rs', 'bg'):
            N = 640 if 'g' in epi else 1280
            plan = dict(family=PP128, stat_parts=24) if 's' in epi else dict(family=PP128)
            out.append(case(f'pp128-sched{sched}-1000x{N}x72-{_epi_tag(epi, 48)}', 1000, N, 72, epi, rpv=48, pad=(0, 8)[sched // 8],
                            opts=dict(gemm_pp=3, pp_sched=sched), plan=plan))
    out.append(case('pp128-28-tiles-stay-on-the-tile-kernels-896x1280x72', 896, 1280, 72, 'b', opts=dict(gemm_pp=3), plan=dict(family=TILE)))
    # what the persistent kernel does not take must show in the plan as leaving it
    out.append(case('pp256-leaves-geglu-alpha-600x160x72', 600, 160, 72, 'bg', alpha=0.25, opts=dict(gemm_pp=4), plan=dict(family=TILE)))
    out.append(case('pp256-leaves-rowvec-residual-600x320x72', 600, 320, 72, 'bvr', rpv=48, opts=dict(gemm_pp=4), plan=dict(family=TILE)))
    out.append(case('pp256-leaves-ldc-pad4-600x320x72', 600, 320, 72, 'br', pad=4, opts=dict(gemm_pp=4), plan=dict(family=TILE)))
    out.append(case('pp256-leaves-rows-per-vec-16-600x320x72', 600, 320, 72, 'bv', rpv=16, opts=dict(gemm_pp=4), plan=dict(family=TILE)))
    return out


def ws_cases():
    out = []
    epis = ('b', 'br', 'bs', 'brs', 'bf', 'bfr', 'bv', 'bfv', '', 'bvs')           # the six compiled epilogues, residual or row vector as the addend
    i = 0
    for waves in (10, 5):
        for M in (32, 64, 96, 32 * 257):
            for N in (320, 640, 960):
                epi = epis[i % len(epis)]
                plan = dict(family=WS, stat_parts=N // 320 * waves) if 's' in epi else dict(family=WS)
                out.append(case(f'ws{waves}-{M}x{N}x320-{_epi_tag(epi, 48)}', M, N, 320, epi, pad=(0, 8)[i % 2], rpv=48,
                                alpha=1.0 if 's' in epi else (1.0, 0.25, 2.0)[i % 3], opts=dict(gemm_pp=1, gemm_ws=2, ws_waves=waves), plan=plan))
                i += 1
        for epi in epis:                          # all of them at one shape, both wave counts
            plan = dict(family=WS, stat_parts=2 * waves) if 's' in epi else dict(family=WS)
            out.append(case(f'ws{waves}-epi-96x640x320-{_epi_tag(epi, 32)}', 96, 640, 320, epi, rpv=32, opts=dict(gemm_pp=1, gemm_ws=2, ws_waves=waves),
                            plan=plan))
    out.append(case('ws-leaves-33-rows', 40, 320, 320, 'b', opts=dict(gemm_pp=1, gemm_ws=2), plan=dict(family=TILE)))
    return out


def conv_cases():
    out = []
    T = dict(gemm_pp=0)

    def cv(tag, conv, N, epi='b', rpv=0, pad=0, opts=T, plan=None, **kw):
        nimg, Hs, Ws, C1, C2, ks, st, ups, lo, hi = conv
        name = (f'conv-{tag}-{nimg}x{Hs}x{Ws}-{C1}+{C2}-k{ks}s{st}' + ('-up' if ups else '') + (f'-pad{lo}{hi}' if lo >= 0 else '') +
                f'-to{N}-{_epi_tag(epi)}' + (f'-ldc+{pad}' if pad else ''))
        out.append(case(name, N=N, epi=epi, rpv=rpv, pad=pad, conv=conv, opts=opts, plan=plan or dict(family=TILE), **kw))

    # 3x3 stride 1, symmetric padding, every image size (1x1: only the centre tap is inside), every C1 (8, 24, 72: a slab straddles taps)
    for i, (Hs, Ws) in enumerate(((1, 1), (1, 5), (2, 2), (3, 5), (5, 3), (7, 9), (8, 8), (16, 16), (32, 32))):
        C1 = (8, 24, 64, 72, 128)[i % 5]
        nimg = (1, 3)[i % 2]
        cv('tile', (nimg, Hs, Ws, C1, 0, 3, 1, 0, -1, -1), (4, 8, 40, 320)[i % 4], ('b', 'bv', 'br', 'bvr')[i % 4], rpv=-1,
           pad=(0, 1, 4, 8)[i % 4])
    for C1 in (8, 24, 64, 72, 128):
        cv('tile', (3, 5, 3, C1, 0, 3, 1, 0, -1, -1), 40, 'bvr', rpv=-1, pad=1)
        cv('tile6', (3, 7, 9, C1, 0, 3, 1, 0, -1, -1), 8, 'br', pad=4, opts=dict(tile_tune=6), plan=_tile_plan(6))
    # two sources (a slab never straddles them: multiples of 64)
    for C1, C2 in ((64, 64), (128, 64)):
        cv('tile', (3, 5, 3, C1, C2, 3, 1, 0, -1, -1), 40, 'bvr', rpv=-2)               # a row vector spanning two images
        cv('tile', (1, 8, 8, C1, C2, 3, 1, 0, -1, -1), 320, 'bv', rpv=-1)
        cv('tile', (3, 7, 9, C1, C2, 1, 1, 0, -1, -1), 8, 'br')
        cv('tile', (1, 3, 5, C1, C2, 3, 1, 1, -1, -1), 40, 'bvr', rpv=-1)               # nearest-2x of a 3x5 source, two sources
        cv('tile', (3, 1, 1, C1, C2, 3, 1, 1, -1, -1), 8, 'b')                          # nearest-2x of a 1x1 source
    # stride 2: odd H or W, the 1x1 stride-2, the paddings (0, 1), (1, 0), (0, 0), (2, 2)
    for Hs, Ws in ((7, 9), (8, 8), (3, 5), (5, 3), (16, 16)):
        cv('tile', (3, Hs, Ws, 72, 0, 3, 2, 0, -1, -1), 40, 'br', pad=1)
        cv('tile', (1, Hs, Ws, 64, 0, 1, 2, 0, -1, -1), 8, 'b')
        for lo, hi in ((0, 1), (1, 0), (0, 0), (2, 2)):
            cv('tile', (3, Hs, Ws, 24, 0, 3, 2, 0, lo, hi), 40, 'bvr', rpv=-1, pad=4)
            cv('tile', (1, Hs, Ws, 64, 64, 3, 1, 0, lo, hi), 8, 'br')
    cv('tile', (3, 1, 5, 8, 0, 3, 2, 0, -1, -1), 4, 'b')
    cv('tile', (3, 1, 1, 64, 0, 1, 2, 0, -1, -1), 320, 'br')
    cv('tile', (1, 1, 1, 64, 0, 1, 1, 0, 0, 0), 4, '')
    # nearest-2x with one source
    for Hs, Ws in ((1, 1), (3, 5)):
        cv('tile', (3, Hs, Ws, 72, 0, 3, 1, 1, -1, -1), 40, 'bvr', rpv=-1, pad=1)
        cv('tile', (1, Hs, Ws, 64, 0, 1, 1, 1, -1, -1), 320, 'b')
    # forced wide tiles and a forced split on a convolution
    cv('tile2', (3, 7, 9, 72, 0, 3, 1, 0, -1, -1), 320, 'bvr', rpv=-1, opts=dict(tile_tune=2), plan=_tile_plan(2))
    cv('tile3', (3, 7, 9, 64, 64, 3, 2, 0, 0, 1), 320, 'br', opts=dict(tile_tune=3), plan=_tile_plan(3))
    cv('split3', (1, 8, 8, 64, 0, 3, 1, 0, -1, -1), 320, 'bvr', rpv=-1, split=True, opts=dict(tile_tune=768),
       plan=dict(family=TILE, BM=128, BN=320, splits=3, nk_per=3))
    cv('split2', (3, 5, 3, 72, 0, 3, 1, 0, -1, -1), 320, 'br', split=True, opts=dict(tile_tune=512),
       plan=dict(family=TILE, BM=128, BN=320, splits=2, nk_per=6))
    # the persistent kernels: C a multiple of 64, every K order (pp_sched 0, 4, 16, 32), both row counts
    for sched in (0, 4, 16, 32):
        P4, P3 = dict(gemm_pp=4, pp_sched=sched), dict(gemm_pp=3, pp_sched=sched)
        cv(f'pp256-sched{sched}', (3, 7, 9, 64, 0, 3, 1, 0, -1, -1), 320, 'bv', rpv=-1, opts=P4, plan=dict(family=PP256))
        cv(f'pp256-sched{sched}', (1, 16, 16, 128, 64, 3, 1, 0, -1, -1), 320, 'br', pad=8, opts=P4, plan=dict(family=PP256))
        cv(f'pp256-sched{sched}', (3, 8, 8, 64, 64, 3, 2, 0, 0, 1), 640, 'b', opts=P4, plan=dict(family=PP256))
        cv(f'pp256-sched{sched}', (1, 3, 5, 64, 0, 3, 1, 1, -1, -1), 320, 'br', opts=P4, plan=dict(family=PP256))
        cv(f'pp256-sched{sched}', (3, 5, 3, 128, 0, 1, 2, 0, -1, -1), 320, 'b', opts=P4, plan=dict(family=PP256))
        cv(f'pp256-sched{sched}', (1, 32, 32, 64, 0, 3, 1, 0, -1, -1), 320, 'bv', rpv=-1, opts=P4, plan=dict(family=PP256))
        cv(f'pp128-sched{sched}', (4, 32, 32, 64, 0, 3, 1, 0, -1, -1), 320, 'br', opts=P3, plan=dict(family=PP128))
        cv(f'pp128-sched{sched}', (17, 16, 16, 64, 64, 3, 1, 0, 2, 2), 320, 'bv', rpv=-2, opts=P3, plan=dict(family=PP128))
    cv('pp256-leaves-C72', (3, 7, 9, 72, 0, 3, 1, 0, -1, -1), 320, 'b', opts=dict(gemm_pp=4), plan=dict(family=TILE))
    return out


def r_cases():
    """Inputs R beyond the GEGLU cases of the tables above (those are R by nature): per family the most ragged shape under every
    epilogue, and a residual 64 x the product"""
    out = []
    for epi in ('bvr', 'bf', 'bfv', 'bt'):
        out.append(case(f'R-tile6-129x65x72-{_epi_tag(epi, 48, 5)}', 129 if 't' not in epi else 130, 65, 72, epi, cls='R', pad=1, rpv=48, rpi=5,
                        alpha=0.25, opts=dict(tile_tune=6), plan=dict(_tile_plan(6), deep=0)))
        out.append(case(f'R-tile18-257x320x136-{_epi_tag(epi, 48, 64)}', 257 if 't' not in epi else 256, 320, 136, epi, cls='R', pad=4 if 't' not in epi else 0,
                        rpv=48, rpi=64, opts=dict(tile_tune=18), plan=dict(_tile_plan(18), deep=0 if 't' in epi else 1)))
    for epi in ('bvr', 'bf', 'bfr'):
        out.append(case(f'R-split3-129x640x264-{_epi_tag(epi, 48)}', 129, 640, 264, epi, cls='R', rpv=48, split=True, opts=dict(tile_tune=768),
                        plan=dict(family=TILE, splits=3, nk_per=2)))
    for epi in ('br', 'bv', 'bf', 'bfv', 'brs', 'bt'):
        M = 512 if 't' in epi else 257
        out.append(case(f'R-pp256-{M}x640x328-{_epi_tag(epi, 48, 256)}', M, 640, 328, epi, cls='R', rpv=48, rpi=256, pad=8, opts=dict(gemm_pp=4),
                        plan=dict(family=PP256)))
    for epi in ('br', 'bv', 'bf', 'bfr', 'brs'):
        out.append(case(f'R-ws10-96x960x320-{_epi_tag(epi, 48)}', 96, 960, 320, epi, cls='R', rpv=48, opts=dict(gemm_pp=1, gemm_ws=2), plan=dict(family=WS)))
    out.append(case('R-conv-tile-3x7x9-72-k3s2-pad01-to40-bvr', N=40, epi='bvr', cls='R', rpv=-1, pad=1, conv=(3, 7, 9, 72, 0, 3, 2, 0, 0, 1),
                    plan=dict(family=TILE)))
    out.append(case('R-conv-pp256-1x3x5-64+64-k3-up-to320-br', N=320, epi='br', cls='R', conv=(1, 3, 5, 64, 64, 3, 1, 1, -1, -1), opts=dict(gemm_pp=4),
                    plan=dict(family=PP256)))
    # a residual 64 x the product: what the product loses under it must still be inside the rule
    out.append(case('R-tile6-residual-x64-129x65x72-br', 129, 65, 72, 'br', cls='R', pad=1, res_scale=64.0, opts=dict(tile_tune=6), plan=_tile_plan(6)))
    out.append(case('R-pp256-residual-x64-257x320x328-br', 257, 320, 328, 'br', cls='R', res_scale=64.0, opts=dict(gemm_pp=4), plan=dict(family=PP256)))
    return out


def refusal_cases():
    """descriptors vsx_gemm_check turns down: the sub-pixel form just below its smallest eligible shape; never launched"""
    sp = lambda nimg, Hs, Ws, C: (nimg, Hs, Ws, C, 0, 3, 1, 2, -1, -1)           # noqa: E731
    return [
        case('refuse-subpixel-128-rows-per-class', N=320, epi='b', conv=sp(1, 8, 16, 64), opts=dict(gemm_pp=4), plan=dict(family=PP256, refused=1), status=-2),
        case('refuse-subpixel-persistent-off', N=320, epi='b', conv=sp(1, 16, 16, 64), opts=dict(gemm_pp=0), plan=dict(family=TILE, refused=1), status=-2),
        case('refuse-subpixel-24-tiles-of-128', N=320, epi='b', conv=sp(3, 16, 16, 64), opts=dict(gemm_pp=3), plan=dict(family=TILE, refused=1), status=-2),
        case('refuse-subpixel-C72', N=320, epi='b', conv=sp(1, 16, 16, 72), opts=dict(gemm_pp=4), plan=dict(family=-1), status=-2),
        case('refuse-subpixel-residual', N=320, epi='br', conv=sp(1, 16, 16, 64), opts=dict(gemm_pp=4), plan=dict(family=-1), status=-2),
    ]


def subpixel_cases():
    """the sub-pixel form at its smallest eligible shape (256 rows per class on the 256-row tiles, 32 tiles of 128), through the raw
    descriptor: B = the four class matrices (`subpixel_weights` below); the reference is the nine-tap form's"""
    sp = lambda nimg, Hs, C: (nimg, Hs, Hs, C, 0, 3, 1, 2, -1, -1)           # noqa: E731
    out = []
    for sched in (0, 4, 16, 32):
        out.append(case(f'subpixel-pp256-sched{sched}-1x16x16-64-to320', N=320, epi='b', conv=sp(1, 16, 64), opts=dict(gemm_pp=4, pp_sched=sched),
                        plan=dict(family=PP256)))
    out.append(case('subpixel-pp256-2x16x16-128-to640', N=640, epi='b', pad=8, conv=sp(2, 16, 128), opts=dict(gemm_pp=4), plan=dict(family=PP256)))
    out.append(case('subpixel-pp128-16x16x16-64-to320', N=320, epi='b', conv=sp(16, 16, 64), opts=dict(gemm_pp=3), plan=dict(family=PP128)))
    return out


TILE_CASES, SPLIT_CASES, PP_CASES, WS_CASES = tile_cases(), split_cases(), pp_cases(), ws_cases()
CONV_CASES, SUBPIXEL_CASES, R_CASES, REFUSALS = conv_cases(), subpixel_cases(), r_cases(), refusal_cases()
ALL_CASES = TILE_CASES + SPLIT_CASES + PP_CASES + WS_CASES + CONV_CASES + SUBPIXEL_CASES + R_CASES
BY_NAME = {c['name']: c for c in ALL_CASES + REFUSALS}
assert len(BY_NAME) == len(ALL_CASES) + len(REFUSALS), 'two cases share a name'
R_NAMES = sorted(c['name'] for c in ALL_CASES if c['cls'] == 'R')


# ------------------------------------------------------------------------------------------------
# input makers
# ------------------------------------------------------------------------------------------------
def _gen(name):
    seed = 0
    for ch in name:
        seed = (seed * 131 + ord(ch)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).to(H)


def _bias_e(g, n, small):
    if small:
        return (2 * torch.randint(-8, 9, (n,), generator=g)).to(H)
    mag = 2 * torch.randint(1024, 2048, (n,), generator=g)
    return (mag * (2 * torch.randint(0, 2, (n,), generator=g) - 1)).to(H)


def subpixel_weights(w):
    """[Cout, 3, 3, C] -> [4, Cout, 3, 3, C]: class (ph, pw) = 2 ph + pw of output pixel (2 i + ph, 2 j + pw); its four taps sit at
    positions (ph.., pw..) of a pad-1 3x3 window on the source and hold the sums of the filter rows / columns that land on the same
    source pixel (include/vsx.h, upsample = 2).  Sums of at most four |w| <= 3: fp16-exact."""
    rows = {0: ((0, (0,)), (1, (1, 2))), 1: ((1, (0, 1)), (2, (2,)))}
    w = w.float()
    out = torch.zeros(4, *w.shape)
    for ph in (0, 1):
        for pw in (0, 1):
            for th, fh in rows[ph]:
                for tw, fw in rows[pw]:
                    out[2 * ph + pw, :, th, tw] = sum(w[:, a, b] for a in fh for b in fw)
    return out.to(H)


class Problem:
    """the tensors of a case on `device` (kept alive here), their host copies, and the descriptor"""


def build(c, device, impl):
    g = _gen(c['name'])
    E = c['cls'] == 'E'
    epi, M, N, K, pad = c['epi'], c['M'], c['N'], c['K'], c['pad']
    cols = 2 * N if 'g' in epi else N
    b0, b1, zero = c['batch'] or (1, 1, False)
    nb = b0 * b1
    pb = Problem()
    pb.c, pb.host, pb.dev = c, {}, {}
    d = pb.d = impl.GemmDesc()
    d.M, d.N, d.K, d.batch0, d.batch1, d.alpha = M, N, K, b0, b1, c['alpha']
    d.geglu = 1 if 'g' in epi else 0
    small = c['small']
    amax = 1 if small else 3

    def put(name, t, offset=0):
        """`t` (flat or not) on the device behind `offset` spare elements -> the address of its first element"""
        flat = t.reshape(-1)
        if offset:
            flat = torch.cat([torch.full((offset,), SENTINEL, dtype=flat.dtype), flat])
        pb.host[name] = flat[offset:].clone().view(t.shape)          # (a tensor of its own: as_strided counts from the storage)
        pb.dev[name] = flat.to(device)
        return pb.dev[name].data_ptr() + offset * flat.element_size()

    def values(lo, hi, *shape, scale=1.0):
        return _ints(g, lo, hi, *shape) if E else (torch.randn(*shape, generator=g) * scale).to(H)

    # ---- A ----
    if c['conv'] is None:
        lda = K + 8
        a_bs1 = M * lda + 8
        a_bs0 = b1 * a_bs1 + 16
        A = torch.full((b0 * a_bs0 + 8,), PAD_VALUE, dtype=H)
        for z0 in range(b0):
            for z1 in range(b1):
                rows = torch.full((M, lda), PAD_VALUE, dtype=H)
                rows[:, :K] = values(-amax, amax, M, K)
                A[z0 * a_bs0 + z1 * a_bs1:][:M * lda] = rows.reshape(-1)
        d.A, d.lda, d.a_bs0, d.a_bs1 = put('A', A), lda, a_bs0 if nb > 1 else 0, a_bs1 if nb > 1 else 0
    else:
        nimg, Hs, Ws, C1, C2, ks, stride, ups, lo, hi = c['conv']
        d.a_mode, d.C1, d.C2, d.ks, d.stride, d.upsample = 1, C1, C2, ks, stride, ups
        d.H, d.W = (2 * Hs, 2 * Ws) if ups else (Hs, Ws)
        d.pad_lo, d.pad_hi = lo, hi
        d.A = put('A', values(-amax, amax, nimg, Hs, Ws, C1))
        if C2:
            d.A2 = put('A2', values(-amax, amax, nimg, Hs, Ws, C2))
    # ---- B: [cols, K] with ldb = K + 8 (the sub-pixel form: four of them, made from the nine-tap weight the reference uses) ----
    ldb = K + 8
    nB = b1 if zero else nb
    w = values(-amax, amax, nB, cols, K, scale=1.0 / math.sqrt(K))
    if small:
        w[:, :, 32:] = 0                       # |acc| <= 32
    pb.host['W'] = w
    subpix = c['conv'] is not None and c['conv'][7] == 2
    wB = subpixel_weights(w[0].view(cols, 3, 3, K // 9)).reshape(1, 4 * cols, K) if subpix else w
    Bt = torch.full((nB, wB.shape[1], ldb), PAD_VALUE, dtype=H)
    Bt[:, :, :K] = wB
    b_bs1 = wB.shape[1] * ldb
    d.B, d.ldb = put('B', Bt), ldb
    if nb > 1:
        d.b_bs1, d.b_bs0 = b_bs1, 0 if zero else b1 * b_bs1
    # ---- epilogue operands ----
    off = 4 if c['align8'] else 0                 # 8-byte aligned, not 16
    if 'b' in epi:
        d.bias = put('bias', _bias_e(g, cols, small) if E else values(0, 0, cols), off)
    if 'v' in epi:
        rpv = c['rpv']
        nvec = (M + rpv - 1) // rpv
        d.rowvec = put('rowvec', values(-16 if small else -2047, 16 if small else 2047, nvec, N), off)
        d.rows_per_vec = rpv
    ldr = N + RPAD[pad]
    if 'r' in epi:
        r_bs1 = M * ldr + 8
        r_bs0 = b1 * r_bs1 + 16
        R = torch.full((b0 * r_bs0 + 8,), PAD_VALUE, dtype=H)
        for z in range(nb):
            rows = torch.full((M, ldr), PAD_VALUE, dtype=H)
            rows[:, :N] = values(-16 if small else -2047, 16 if small else 2047, M, N, scale=c['res_scale'])
            R[(z // b1) * r_bs0 + (z % b1) * r_bs1:][:M * ldr] = rows.reshape(-1)
        d.residual, d.ldr = put('R', R, off), ldr
        if nb > 1:
            d.r_bs0, d.r_bs1 = r_bs0, r_bs1
    if 'f' in epi:
        if E:
            rs = torch.stack([torch.exp2(torch.randint(-2, 2, (M,), generator=g).float()), torch.randint(-3, 4, (M,), generator=g).float()], dim=1)
            cv = torch.randint(-8, 9, (cols,), generator=g).float()
        else:                                     # the statistics and c1 of ops.DeferredLN, formed as it forms them (fp32)
            x = pb.host['A'][:M * (K + 8)].view(M, K + 8)[:, :K].float()
            var, mean = torch.var_mean(x, dim=-1, unbiased=False)
            rstd = (var + 1e-5).rsqrt()
            rs = torch.stack([rstd, -rstd * mean], dim=1)
            cv = w[0].float().sum(1)
        d.rowscale, d.colvec = put('rowscale', rs.contiguous()), put('colvec', cv.contiguous())
    # ---- C inside its guard band ----
    ldc = N + pad
    if 't' in epi:
        rpi = c['rpi']
        assert M % rpi == 0
        ldc = round_up(rpi, 8) + 8
        d.c_mode, d.c_rows_per_img, d.c_img_stride = 1, rpi, N * ldc + 24
        span = (M // rpi) * d.c_img_stride
        idx = (torch.arange(M) // rpi * d.c_img_stride + torch.arange(M) % rpi)[:, None] + torch.arange(N)[None, :] * ldc
        idx = idx[None]
    else:
        c_bs1 = round_up((M + 1) * ldc, 8)
        c_bs0 = b1 * c_bs1 + 16
        span = (b0 - 1) * c_bs0 + (b1 - 1) * c_bs1 + M * ldc
        z = torch.arange(nb)
        idx = ((z // b1) * c_bs0 + (z % b1) * c_bs1)[:, None, None] + torch.arange(M)[None, :, None] * ldc + torch.arange(N)[None, None, :]
        if nb > 1:
            d.c_bs0, d.c_bs1 = c_bs0, c_bs1
    coff = round_up(4 * ldc, 8)
    pb.cidx = (idx + coff).reshape(nb, M, N)                       # where element (z, m, n) of the result lives in the buffer
    pb.cbuf = torch.full((coff + span + 4 * ldc + 8,), SENTINEL, dtype=H).to(device)
    d.C, d.ldc = pb.cbuf.data_ptr() + 2 * coff, ldc
    # ---- row statistics, split-K workspace ----
    if 's' in epi:
        parts = impl.rowstats_parts(d)
        pb.stats = torch.full((M, max(parts, 1), 2), float('nan'), dtype=torch.float32).to(device)
        d.rowstats, d.rowstats_parts = pb.stats.data_ptr(), parts
    if c['split']:
        need = impl.workspace(d)
        assert need > 0, (c['name'], 'vsx_gemm_workspace: this descriptor does not split')
        pb.ws = torch.zeros(need // 4 + 4, dtype=torch.float32).to(device)
        d.workspace, d.workspace_bytes = pb.ws.data_ptr(), need
    return pb


# ------------------------------------------------------------------------------------------------
# the reference, on the descriptor: every field the tables use, plain PyTorch in `dt`
# ------------------------------------------------------------------------------------------------
def _im2col(d, x1, x2, dt):
    """the A matrix [M, ks * ks * (C1 + C2)] of an a_mode 1 descriptor: K runs (kh, kw, [source 1 | source 2])"""
    ks, st = d.ks, d.stride
    lo, hi = (ks // 2, ks // 2) if d.pad_lo < 0 else (d.pad_lo, d.pad_hi)
    x = x1.to(dt) if x2 is None else torch.cat([x1.to(dt), x2.to(dt)], dim=-1)
    if d.upsample:
        x = x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    assert x.shape[1] == d.H and x.shape[2] == d.W
    x = F.pad(x, (0, 0, lo, hi, lo, hi))
    Ho, Wo = (d.H + lo + hi - ks) // st + 1, (d.W + lo + hi - ks) // st + 1
    taps = [x[:, kh:kh + (Ho - 1) * st + 1:st, kw:kw + (Wo - 1) * st + 1:st, :] for kh in range(ks) for kw in range(ks)]
    return torch.cat(taps, dim=-1).reshape(d.M, d.K)


def _gelu(g):
    return 0.5 * g * (1.0 + torch.erf(g * 0.7071067811865476))


def _dgelu(g):
    return 0.5 * (1.0 + torch.erf(g * 0.7071067811865476)) + g * torch.exp(-0.5 * g * g) * 0.3989422804014327


def chain(pb, dt, absolute=False):
    """[batch, M, N] in `dt`: alpha, the fold, the bias, GEGLU (erf form), the row vector, the residual last.  absolute: the same
    chain over the absolute values of every term (S of the rule; GEGLU propagates it to first order, around the fp64 h and g)"""
    d, hst, c = pb.d, pb.host, pb.c
    epi, M, N, K = c['epi'], d.M, d.N, d.K
    nb, b1 = d.batch0 * d.batch1, d.batch1
    ab = (lambda t: t.abs()) if absolute else (lambda t: t)
    outs = []
    for z in range(nb):
        z0, z1 = z // b1, z % b1
        if d.a_mode == 0:
            A = torch.as_strided(hst['A'], (M, K), (d.lda, 1), z0 * d.a_bs0 + z1 * d.a_bs1).to(dt)
        else:
            up = 1 if d.upsample == 2 else d.upsample             # the sub-pixel form computes the nine-tap convolution
            dd = type('D', (), dict(ks=d.ks, stride=d.stride, pad_lo=d.pad_lo, pad_hi=d.pad_hi, upsample=up, H=d.H, W=d.W, M=M, K=K))
            A = _im2col(dd, hst['A'], hst.get('A2'), dt)
        W = hst['W'][z1 if c['batch'] and c['batch'][2] else z].to(dt)          # [cols, K] (the B operand without its pad columns)
        acc = ab(A) @ ab(W).t() * abs(d.alpha) if absolute else A @ W.t() * d.alpha
        if 'f' in epi:
            rs, cv = hst['rowscale'].to(dt), hst['colvec'].to(dt)
            acc = ab(rs[:, :1]) * acc + ab(rs[:, 1:]) * ab(cv)[None, :]
        if 'b' in epi:
            acc = acc + ab(hst['bias'].to(dt))[None, :]
        if 'g' in epi:
            if absolute:
                hv, gv = pb.pre_geglu[z]
                acc = _gelu(gv).abs() * acc[:, :N] + hv.abs() * _dgelu(gv).abs() * acc[:, N:]
            else:
                if dt == torch.float64:
                    pb.pre_geglu = getattr(pb, 'pre_geglu', {})
                    pb.pre_geglu[z] = (acc[:, :N], acc[:, N:])
                acc = acc[:, :N] * _gelu(acc[:, N:])
        if 'v' in epi:
            acc = acc + ab(hst['rowvec'].to(dt))[torch.arange(M) // d.rows_per_vec]
        if 'r' in epi:
            acc = acc + ab(torch.as_strided(hst['R'], (M, N), (d.ldr, 1), z0 * d.r_bs0 + z1 * d.r_bs1).to(dt))
        outs.append(acc)
    return torch.stack(outs)


def elem_extra(pb, want):
    """the per-element room of Inputs R beyond the output's own fp16 ulp (module docstring)"""
    extra = 2.0 ** -10 * want.pow(2).mean(-1, keepdim=True).sqrt() + (pb.d.K + 4) * 2.0 ** -24 * chain(pb, torch.float64, absolute=True)
    if 'g' in pb.c['epi']:
        hv = torch.stack([pb.pre_geglu[z][0] for z in sorted(pb.pre_geglu)]).abs()
        gv = torch.stack([pb.pre_geglu[z][1] for z in sorted(pb.pre_geglu)]).abs()
        extra = extra + 1e-5 * hv * torch.maximum(torch.ones_like(gv), gv)
    return extra


# ------------------------------------------------------------------------------------------------
# the rule and the runners
# ------------------------------------------------------------------------------------------------
def assert_plan(impl, pb):
    c = pb.c
    rc, plan = impl.plan(pb.d)
    assert rc == c['status'] == impl.check(pb.d), (c['name'], rc, plan)
    for k, v in c['plan'].items():
        assert plan[k] == v, (c['name'], f'aimed at {k} = {v}', plan)
    return plan


def _bits(t):
    return t.contiguous().view(torch.int16)


def check_guards(pb, before, after):
    """everything in C's buffer outside the result is bit-identical to before"""
    outside = torch.ones(after.numel(), dtype=torch.bool)
    outside[pb.cidx.reshape(-1)] = False
    moved = (_bits(after) != _bits(before)) & outside
    assert not bool(moved.any()), (pb.c['name'], 'stored outside the result', int(moved.sum()),
                                   'first at element', int(moved.nonzero()[0]) - int(pb.cidx.min()), 'from C')


def check_exact(pb, got, stats=None):
    c = pb.c
    want = chain(pb, torch.float64)
    want16 = want.to(H)
    assert bool((want16.double() == want).all()) or not c['small'], c['name']            # (small cases: no rounding at all)
    diff = _bits(got) != _bits(want16)
    fig = dict(case=c['name'], cls='E', elements=got.numel(), mismatches=int(diff.sum()),
               ties=int(((want - want16.double()).abs() * 2 == tk.ulp16(want)).sum()))
    if stats is not None:
        o = want16.double()[0]
        assert bool(o.abs().max() <= 64), c['name']
        tot = stats.double().sum(1)
        bad = (tot[:, 0] != o.sum(1)) | (tot[:, 1] != o.pow(2).sum(1)) | ~torch.isfinite(stats.double()).all(-1).all(-1)
        fig['stat_rows_wrong'] = int(bad.sum())
    FIGURES.append(fig)
    if diff.any():
        where = diff.nonzero()[0].tolist()
        assert False, (c['name'], f'{int(diff.sum())} of {got.numel()} elements differ from the once-rounded fp64 result; first (z, m, n) = {where}',
                       float(got[tuple(where)]), float(want[tuple(where)]))
    assert fig.get('stat_rows_wrong', 0) == 0, (c['name'], 'row statistics', fig)
    return fig


def check_rounded(pb, got, stats=None):
    c = pb.c
    want = chain(pb, torch.float64)
    ideal = chain(pb, torch.float32).to(H)
    fig, failed = measure(got, want, ideal, elem_extra(pb, want))
    fig = dict(case=c['name'], cls='R', **fig)
    if stats is not None:                      # fp32 sums of the ROUNDED outputs the launch stored: up to N roundings of the running sum
        o = got.double()[0]
        tot = stats.double().sum(1)
        fig['stat_sum_err'] = float(((tot[:, 0] - o.sum(1)).abs() / o.abs().sum(1).clamp_min(1e-30)).max())
        fig['stat_sq_err'] = float(((tot[:, 1] - o.pow(2).sum(1)).abs() / o.pow(2).sum(1).clamp_min(1e-30)).max())
        fig['stat_bound'] = (c['N'] + 4) * 2.0 ** -24
        if not (fig['stat_sum_err'] <= fig['stat_bound'] and fig['stat_sq_err'] <= fig['stat_bound']):
            failed.append('rowstats')
    print(' '.join(f'{k}={v:.3e}' if isinstance(v, float) else f'{k}={v}' for k, v in fig.items()))
    FIGURES.append(fig)
    assert not failed, (c['name'], failed, fig)
    return fig


def run_case(impl, device, c):
    with options(impl, c['opts']):
        pb = build(c, device, impl)
        assert_plan(impl, pb)
        if c['status'] != 0:
            return None
        before = pb.cbuf.cpu().clone()
        impl.gemm(pb.d)
        impl.sync()
        after = pb.cbuf.cpu()
        got = after[pb.cidx]
        stats = pb.stats.cpu() if 's' in c['epi'] else None
        fig = (check_exact if c['cls'] == 'E' else check_rounded)(pb, got, stats)
        check_guards(pb, before, after)
        return fig


def expected_figures():
    return len(ALL_CASES)


# ------------------------------------------------------------------------------------------------
# the wrappers' own arithmetic: ops.linear(out=), ops.linear_vt(ldvt=), ops.conv2d in both forms, ops.DeferredLN
# ------------------------------------------------------------------------------------------------
WRAPPER_RUNS = ['linear-out-guarded', 'linear-vt-ldvt', 'conv2d-nine-tap-equals-subpixel', 'deferred-ln-tile', 'deferred-ln-pp256',
                'deferred-ln-ws', 'deferred-ln-split', 'deferred-ln-vt']


def run_wrapper(impl, device, name):
    g = _gen(name)
    dev = lambda t: t.to(device)                  # noqa: E731
    if name == 'linear-out-guarded':
        with options(impl, dict(tile_tune=6)):
            M, N, K = 70, 44, 72
            x, w, b, r = _ints(g, -3, 3, M, K), _ints(g, -3, 3, N, K), _bias_e(g, N, False), _ints(g, -2047, 2047, M, N)
            buf = dev(torch.full((M + 8, N), SENTINEL, dtype=H))
            y = impl.linear(dev(x), dev(w), dev(b), residual=dev(r), out=buf[4:4 + M])
            impl.sync()
            want = (x.double() @ w.double().t() + b.double() + r.double()).to(H)
            assert y.data_ptr() == buf[4:].data_ptr()
            assert torch.equal(_bits(buf[4:4 + M].cpu()), _bits(want)), name
            assert bool((buf[:4].cpu() == SENTINEL).all()) and bool((buf[4 + M:].cpu() == SENTINEL).all()), name
    elif name == 'linear-vt-ldvt':
        with options(impl, dict(tile_tune=6)):
            rows, nimg, N, K, ldvt = 77, 2, 40, 72, 96
            x, w, b = _ints(g, -3, 3, nimg * rows, K), _ints(g, -3, 3, N, K), _bias_e(g, N, False)
            vt = impl.linear_vt(dev(x), dev(w), dev(b), rows, ldvt=ldvt).cpu()
            want = (x.double() @ w.double().t() + b.double()).to(H).view(nimg, rows, N).transpose(1, 2)
            assert vt.shape == (nimg, N, ldvt) and torch.equal(_bits(vt[:, :, :rows]), _bits(want)), name
            assert bool((vt[:, :, rows:] == 0).all()), name                      # the wrapper zero-fills what the kernel must not touch
    elif name == 'conv2d-nine-tap-equals-subpixel':
        with options(impl, dict(gemm_pp=4)):
            x, w, b = _ints(g, -3, 3, 1, 16, 16, 64), _ints(g, -3, 3, 320, 3, 3, 64), _bias_e(g, 320, False)
            xd, wd, bd = dev(x), dev(w), dev(b)
            nine = impl.conv2d_form(False, xd, wd, bd, upsample=True).cpu()
            sub = impl.conv2d_form(True, xd, wd, bd, upsample=True).cpu()
            up = x.double().repeat_interleave(2, 1).repeat_interleave(2, 2).permute(0, 3, 1, 2)
            want = (F.conv2d(up, w.double().permute(0, 3, 1, 2), b.double(), padding=1)).permute(0, 2, 3, 1).to(H)
            assert torch.equal(_bits(nine), _bits(want)), (name, 'nine-tap form')
            assert torch.equal(_bits(sub), _bits(want)), (name, 'sub-pixel form')
    else:
        kind = name.rsplit('-', 1)[1]
        opts, M, N, K = {'tile': (dict(tile_tune=6), 129, 72, 72), 'pp256': (dict(gemm_pp=4), 257, 640, 328),
                         'ws': (dict(gemm_pp=1, gemm_ws=2), 96, 640, 320), 'split': (dict(tile_tune=768), 129, 320, 832),
                         'vt': (dict(tile_tune=6), 154, 72, 72)}[kind]
        with options(impl, opts):
            x = (torch.randn(M, K, generator=g) * 1.5 + 0.3).to(H)
            gamma, beta = (1 + 0.1 * torch.randn(K, generator=g)).to(H), (0.1 * torch.randn(K, generator=g)).to(H)
            w, b = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(H), torch.randn(N, generator=g).to(H)
            ln = impl.DeferredLN(dev(x), dev(gamma), dev(beta), 1e-5)
            if kind == 'vt':
                got = impl.linear_vt(ln, dev(w), dev(b), 77).cpu()[:, :, :77].transpose(1, 2).reshape(M, N)
            else:
                got = impl.linear(ln, dev(w), dev(b)).cpu()
            impl.sync()

            # what the wrapper hands the launch (ops._ln_folded, restated): W' = W o gamma and c2 = beta W^T + b rounded to fp16, c1 =
            # the row sums of W' in fp32; the statistics are those of x.  The chain on those: rs acc + rt c1 + c2
            w32 = w.float()
            wf = (w32 * gamma.float()[None, :]).to(H)
            c1, c2 = wf.float().sum(1), (w32 @ beta.float() + b.float()).to(H)

            def ref(dt):
                var, mean = torch.var_mean(x.to(dt), dim=-1, unbiased=False, keepdim=True)
                rstd = (var + 1e-5).rsqrt()
                return rstd * (x.to(dt) @ wf.to(dt).t()) + (-rstd * mean) * c1.to(dt)[None, :] + c2.to(dt)[None, :]
            want = ref(torch.float64)
            xd = x.double()
            var, mean = torch.var_mean(xd, dim=-1, unbiased=False, keepdim=True)
            rstd = (var + 1e-5).rsqrt()
            S = rstd * (xd.abs() @ wf.double().abs().t() + mean.abs() * c1.double().abs()[None, :]) + c2.double().abs()[None, :]
            extra = 2.0 ** -10 * want.pow(2).mean(-1, keepdim=True).sqrt() + (K + 4) * 2.0 ** -24 * S
            fig, failed = measure(got, want, ref(torch.float32).to(H), extra)
            fig = dict(case=name, cls='R', **fig)
            print(' '.join(f'{k}={v:.3e}' if isinstance(v, float) else f'{k}={v}' for k, v in fig.items()))
            FIGURES.append(fig)
            assert not failed, (name, failed, fig)
