"""Shared pieces of tests/test_winograd.py (CPU) and tests/test_winograd_gpu.py: a torch restatement of the three stages of
include/vsx.h's vsx_conv3x3_winograd_f16 with the same rounding points (fp32 transform arithmetic; V, U, Mt and the output
rounded to fp16 once each), and the inputs both files use (SiLU-shaped activations, weights ~ N(0, 1 / K))."""
import torch
import torch.nn.functional as F

BT = torch.tensor([[1., 0., -1., 0.], [0., 1., 1., 0.], [0., -1., 1., 0.], [0., 1., 0., -1.]])
AT = torch.tensor([[1., 1., 1., 0.], [0., 1., -1., -1.]])
G = torch.tensor([[1., 0., 0.], [.5, .5, .5], [.5, -.5, .5], [0., 0., 1.]])

REL_L2_BOUND = 2e-3          # the project's bound for a convolution (tests/test_kernels_gpu.py)
RATIO_BOUND = 3.0            # at most 3 x the direct form's error on the same inputs


def make_case(nimg, H, W, C1, C2, Cout, rowvec=False, residual=False, seed=0):
    """fp16 tensors of one convolution: x [nimg, H, W, C1] (+ x2), weight [Cout, 3, 3, C1 + C2], bias [Cout], optionally a
    row vector per image ([nimg, Cout], rows_per_vec = H * W) and a residual [nimg, H, W, Cout]."""
    g = torch.Generator().manual_seed(seed)
    C = C1 + C2
    x = F.silu(torch.randn(nimg, H, W, C, generator=g)).half()      # SiLU of a GroupNorm output: unit variance in front of it
    case = dict(x=x[..., :C1].contiguous(), x2=x[..., C1:].contiguous() if C2 else None,
                weight=(torch.randn(Cout, 3, 3, C, generator=g) / (9 * C) ** 0.5).half(),
                bias=(torch.randn(Cout, generator=g) * 0.1).half(),
                rowvec=(torch.randn(nimg, Cout, generator=g) * 0.3).half() if rowvec else None,
                residual=torch.randn(nimg, H, W, Cout, generator=g).half() if residual else None,
                rows_per_vec=H * W)
    return case


def reference(case, dtype=torch.float64):
    """F.conv2d on the fp16 values in `dtype`, then bias, row vector and residual: [nimg, H, W, Cout]"""
    x = case['x'] if case['x2'] is None else torch.cat([case['x'], case['x2']], -1)
    y = F.conv2d(x.to(dtype).permute(0, 3, 1, 2), case['weight'].to(dtype).permute(0, 3, 1, 2), padding=1).permute(0, 2, 3, 1)
    y = y + case['bias'].to(dtype)
    if case['rowvec'] is not None:
        y = y + case['rowvec'].to(dtype)[:, None, None, :]
    if case['residual'] is not None:
        y = y + case['residual'].to(dtype)
    return y


def direct_fp16(case):
    """what the direct form can do at best: the fp64 result rounded to fp16 once"""
    return reference(case).half()


def input_transform(x):
    """x fp16 [nimg, H, W, C] -> V fp16 [16, nimg * H/2 * W/2, C]"""
    nimg, H, W, C = x.shape
    xp = F.pad(x.float(), (0, 0, 1, 1, 1, 1))
    d = xp.unfold(1, 4, 2).unfold(2, 4, 2)                       # [nimg, H/2, W/2, C, 4 (rows), 4 (columns)]
    v = torch.einsum('ar,nijcrs,bs->abnijc', BT, d, BT)
    return v.reshape(16, -1, C).half()


def weight_transform(weight):
    """[Cout, 3, 3, C] fp16 -> U fp16 [16, Cout, C]"""
    u = torch.einsum('ar,orsc,bs->aboc', G, weight.float(), G)
    return u.reshape(16, weight.shape[0], weight.shape[3]).half()


def output_transform(mt, nimg, H, W):
    """Mt fp16 [16, tiles, Cout] -> fp32 [nimg, H, W, Cout] (before the epilogue)"""
    m = mt.float().reshape(4, 4, nimg, H // 2, W // 2, -1)
    y = torch.einsum('pa,abnijo,qb->nipjqo', AT, m, AT)
    return y.reshape(nimg, H, W, -1)


def winograd_restated(case):
    """the three stages with the kernels' rounding points -> fp16 [nimg, H, W, Cout]"""
    x = case['x'] if case['x2'] is None else torch.cat([case['x'], case['x2']], -1)
    nimg, H, W, _ = x.shape
    v = input_transform(x)
    u = weight_transform(case['weight'])
    mt = torch.bmm(v.float(), u.float().transpose(1, 2)).half()          # fp32 sums of fp16 products, one rounding
    y = output_transform(mt, nimg, H, W)
    y = y + case['bias'].float()
    if case['rowvec'] is not None:
        y = y + case['rowvec'].float()[:, None, None, :]
    if case['residual'] is not None:
        y = y + case['residual'].float()
    return y.half()


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


# ================================================================================================
# Stage-by-stage parity of vsx_conv3x3_winograd_f16 at tile edges: shared by tests/test_winograd_kernels_gpu.py (the HIP kernels
# of videoswap_amd/csrc/winograd.hip and the batched vsx_gemm_f16 launch between them) and tests/test_winograd_case.py (a CPU
# restatement of the entry point on the descriptor, and deliberate mutants of it).  No kernels and no GPU calls in this file:
# every runner takes `impl` (launch of the entry point from a descriptor, the workspace query, option get / set, sync) and a
# device.  The runner builds the GemmDesc itself, so it owns ldc, ldr, rows_per_vec and the workspace.
#
# The workspace (V [16][M/4][C1+C2], then Mt [16][M/4][N], include/vsx.h) belongs to the caller and is never cleared, so both are
# read back after the call and every stage is judged on the KERNEL'S OWN input to that stage.
#
#   E (exact)    x, x2 integers in [-ax, ax], weights integers in [-aw, aw] (`amp`, (3, 2) unless the channel count asks for
#                (1, 1)); bias EVEN integers with 2048 <= |b| <= 4094; row vector and residual integers in [-2047, 2047].  V is then
#                an integer, U and Mt multiples of 1/4, all fp16-exact (`exact_stages` asserts it, in fp64, for every case: a case
#                that does not meet it is an error in the table), the pre-epilogue output is the true convolution, and every
#                epilogue partial sum stays below 2^24: every summation order gives the same number.
#   R (rounded)  the Gaussian inputs of `make_case` (SiLU-shaped activations, weights ~ N(0, 1 / K)); `res_scale` = 64: a residual
#                64 x the rms of the product.
# ================================================================================================
import contextlib
import ctypes
import time

import gemm_case as gc
import train_kernel_case as tk
from train_kernel_case import measure

H16 = torch.float16
SENTINEL = gc.SENTINEL
VSX_OK, VSX_E_UNSUPPORTED, VSX_E_WORKSPACE = 0, -2, -4
WS_GUARD = 512                  # sentinel elements in front of and behind the workspace (more than one tile row of any case)
C_GUARD_ROWS = 4                # sentinel rows in front of and behind C
FIGURES = []                    # one dict per case run
# every option a case may depend on, with the value the tables start from: the library's defaults, the form forced
BASE_OPTS = dict(gemm_pp=1, gemm_ws=1, ws_waves=10, tile_tune=0, pp_sched=0, xcd_walk=1, conv_winograd=2)
RPAD = {0: 8, 8: 0, 16: 24}     # ldr = N + RPAD[pad]: never ldc, above and below it
RULE = ('Every case reads V and Mt back from the workspace.  U: E bit-equal to fp64 G g G^T; R within half an fp16 ulp + 9 * 2^-24 * '
        'sum |terms| of it.  V: bit-equal to the fp32 restatement of B^T d B in the written order (columns first: d0 - d2, d1 + d2, '
        'd2 - d1, d1 - d3; then rows; one rounding); E also bit-equal to fp64.  Mt: E bit-equal to fp64 bmm(V, U^T); R '
        'train_kernel_case.measure (l2 <= 1.5 ideal, worst row <= 2 ideal, max-abs <= 4 ideal, per element <= 1 fp16 ulp + extra) '
        'against fp64 bmm of the kernel\'s own V and U, ideal = the fp32 bmm rounded once, extra = 2^-10 rms(row) + (K + 4) 2^-24 S, '
        'S = sum |v||u|.  Y: bit-equal to the fp32 restatement of A^T Mt A (m0 + m1 + m2 and m1 - m2 - m3 down the columns, then '
        'along the rows) + bias + row vector + residual, one rounding, from the kernel\'s own Mt; E also bit-equal to the fp64 '
        'convolution + epilogue rounded once.  R end to end: rel-L2 against the fp64 convolution < 2e-3 and <= 3 x the direct form '
        'on the same inputs.  C and the workspace (exactly the bytes the library asks for) lie inside sentinel-filled buffers; '
        'every byte outside the result and the workspace, the inputs included, is unchanged; two calls give the same bits.')


class WinoQueries(gc.LibQueries):
    """gemm_case.LibQueries plus the Winograd form's host-side query.  A subclass adds winograd(d, u_ptr, ws_ptr, ws_bytes) -> rc,
    gemm(d) (the direct form of the same description), winograd_weights(w), conv2d(...) and sync()."""

    def wino_workspace(self, d):
        return int(self.lib().vsx_conv3x3_winograd_workspace(ctypes.byref(d)))

    def batched_family(self, c):
        """the kernel family (gemm_case.WS / PP256 / PP128 / TILE) that carries the batched launch of `c` under the current options"""
        rc, plan = self.plan(batched_desc(self, c))
        assert rc == 0, (c['name'], rc)
        return plan['family']


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
def wcase(edge, nimg, H, W, C1, C2, N, epi='bvr', rpv='HW', pad=0, cls='E', amp=(3, 2), pad11=False, opts=None, res_scale=0.0):
    """epi: letters b(ias) v(row vector) r(esidual).  rpv: 'HW', '2HW', 'W' or a number.  pad: ldc = N + pad.  pad11: pad_lo =
    pad_hi = 1 written out instead of -1.  edge: what the case is aimed at (the start of its name)."""
    rows = {'HW': H * W, '2HW': 2 * H * W, 'W': W}.get(rpv, rpv)
    name = (f'{edge}-{cls}-{nimg}x{H}x{W}-{C1}+{C2}-to{N}-{epi or "none"}' + (f'-rpv{rpv}' if 'v' in epi else '') + f'-ldc+{pad}' +
            ('-pad11' if pad11 else '') + ''.join(f'-{k}{v}' for k, v in sorted((opts or {}).items())) + ('-residual-x64' if res_scale else ''))
    return dict(name=name, edge=edge, nimg=nimg, H=H, W=W, C1=C1, C2=C2, N=N, epi=epi, rpv=rows, pad=pad, cls=cls, amp=amp, pad11=pad11,
                opts=dict(opts or {}), res_scale=res_scale, M=nimg * H * W, tiles=nimg * H * W // 4)


def case_id(c):
    return c['name']


def geometry_cases():
    return [
        wcase('one-tile-all-taps-outside-the-interior-are-padding', 1, 2, 2, 8, 0, 8),
        wcase('one-tile-per-image', 3, 2, 2, 8, 0, 8, rpv='2HW', pad=8),
        wcase('one-tile-row-wide', 1, 2, 16, 8, 0, 8, 'br', pad=16),
        wcase('one-tile-column-tall', 1, 16, 2, 8, 0, 8, 'bv', rpv='W'),
        wcase('wider-than-tall', 3, 4, 6, 64, 0, 64, pad=8),
        wcase('taller-than-wide', 3, 6, 4, 64, 0, 64, pad=16),
        wcase('taller-than-wide-one-tile-column', 1, 6, 2, 72, 0, 24),
        wcase('square-two-images', 2, 8, 8, 128, 0, 64, 'br', pad=8),
        # tile counts against the GEMM's 128-row tile
        wcase('127-tiles', 1, 2, 254, 8, 0, 8, 'b'),
        wcase('128-tiles', 1, 16, 32, 8, 0, 8, 'br', pad=8),
        wcase('129-tiles', 3, 2, 86, 72, 0, 24, pad=16),
        wcase('129-tiles', 3, 2, 86, 8, 0, 72, 'bv', rpv='W'),
        # threads against the 256-thread workgroup: tiles * C / 8 (input transform) and tiles * N / 8 (output transform)
        wcase('255-threads-in-and-out', 1, 2, 510, 8, 0, 8, 'r'),
        wcase('256-threads-in-and-out-exactly', 1, 16, 32, 16, 0, 16, 'bv', rpv=3, pad=8),
        wcase('256-threads-out-exactly', 1, 8, 16, 8, 0, 64, 'b'),
        wcase('257-threads-in-and-out', 1, 2, 514, 8, 0, 8, 'br', pad=16),
        wcase('513-threads-in-257-out', 1, 2, 514, 16, 0, 8, 'bv', rpv=1),
        wcase('partial-last-workgroup-many-octets', 3, 2, 86, 136, 0, 72, 'br', pad=8),
    ]


def channel_cases():
    out = []
    for i, (C, N) in enumerate(((8, 8), (8, 72), (64, 24), (64, 64), (72, 8), (72, 72), (136, 24), (136, 64))):
        out.append(wcase(f'K{C}', (1, 3)[i % 2], (4, 6)[i % 2], (6, 4)[i % 2], C, 0, N, ('bvr', 'br', 'bv', 'b')[i % 4], pad=(0, 8, 16)[i % 3]))
    # two sources: a source stride mixed up between them shows only when they differ
    out.append(wcase('two-sources', 3, 4, 6, 64, 128, 24, pad=8))
    out.append(wcase('two-sources', 3, 4, 6, 128, 64, 24, pad=16))
    out.append(wcase('two-sources', 1, 2, 2, 64, 128, 8, 'b'))
    # the model's channel counts at a tiny image: amplitudes {-1, 0, 1}
    out.append(wcase('deep-level-channels', 1, 4, 4, 1280, 0, 64, amp=(1, 1)))
    out.append(wcase('deep-level-channels-two-sources', 1, 4, 4, 576, 64, 64, 'br', pad=8, amp=(1, 1)))
    return out


def epilogue_cases():
    out = []
    for i, epi in enumerate(('', 'b', 'v', 'r', 'bv', 'br', 'vr', 'bvr')):          # every subset
        out.append(wcase('epilogue', 3, 4, 6, 8, 0, 24, epi, pad=(0, 8, 16)[i % 3]))
        out.append(wcase('epilogue', 1, 6, 4, 72, 0, 8, epi, rpv='W', pad=(8, 16, 0)[i % 3]))
    # rows_per_vec: W gives the two rows of a tile different vectors, 3 the two columns; 2 H W spans two of three images
    for i, rpv in enumerate(('HW', '2HW', 'W', 3, 1)):
        out.append(wcase('rows-per-vec', 3, 4, 6, 8, 0, 24, 'bv', rpv=rpv, pad=(0, 8, 16)[i % 3]))
        out.append(wcase('rows-per-vec', 3, 6, 4, 72, 0, 8, 'bvr', rpv=rpv, pad=(16, 0, 8)[i % 3]))
    out.append(wcase('padding-written-out', 3, 4, 6, 8, 0, 24, pad11=True))
    out.append(wcase('padding-written-out', 1, 2, 2, 72, 0, 8, 'b', pad=8, pad11=True))
    # the tie cases: acc + bias sits where fp16 steps by 2 and every odd sum is a tie.  Bias alone (acc is an fp16-exact integer, so
    # only a rounding of acc + bias itself can go wrong), and with the other two terms (a bias added after THEIR sum was rounded)
    out.append(wcase('bias-ties', 3, 4, 6, 64, 0, 64, 'b'))
    out.append(wcase('bias-ties', 3, 4, 6, 64, 0, 64, 'bvr', rpv=1))
    # both GEMM back ends under the raw entry point
    out.append(wcase('gemm-back-end', 3, 4, 6, 72, 0, 24, opts=dict(gemm_pp=0)))
    return out


def rounded_cases():
    R = dict(cls='R')
    return [
        wcase('resnet-conv1', 3, 4, 6, 64, 0, 64, 'bv', **R),
        wcase('resnet-conv2', 3, 4, 6, 64, 0, 64, 'br', pad=8, **R),
        wcase('K-tail', 2, 8, 8, 72, 0, 72, 'bvr', rpv='W', pad=16, **R),
        wcase('K136', 3, 6, 4, 136, 0, 24, 'bv', rpv=3, **R),
        wcase('two-sources', 3, 4, 6, 64, 128, 24, 'bvr', pad=8, **R),
        wcase('two-sources', 1, 8, 8, 128, 64, 64, 'br', **R),
        wcase('129-tiles', 3, 2, 86, 72, 0, 24, 'bvr', rpv='2HW', pad=16, **R),
        # (the ratio to the direct form is a statistic over the elements: 1 x 4 x 4 x 64 of them leave it a spread of several per
        # cent around its expectation of 2.7, which is what separates that from the bound of 3; 4096 elements here)
        wcase('deep-level-channels', 1, 8, 8, 640, 0, 64, 'bv', **R),
        wcase('one-tile', 1, 2, 2, 64, 0, 8, 'br', **R),
        wcase('gemm-back-end', 2, 8, 8, 72, 0, 72, 'br', opts=dict(gemm_pp=0), **R),
        wcase('resnet-conv2', 3, 4, 6, 64, 0, 64, 'br', pad=8, res_scale=64.0, **R),
        wcase('two-sources', 1, 8, 8, 128, 64, 64, 'br', res_scale=64.0, **R),
    ]


def wrapper_cases():
    """through ops.conv2d under conv_winograd = 2 with x2, a row vector and a residual; both GEMM back ends"""
    return [
        wcase('conv2d', 3, 4, 6, 64, 128, 24, rpv='HW', opts=dict(gemm_pp=0)),
        wcase('conv2d', 3, 4, 6, 128, 64, 24, rpv='2HW', opts=dict(gemm_pp=1)),
        wcase('conv2d', 1, 2, 2, 64, 64, 8, rpv=3, opts=dict(gemm_pp=1)),
        wcase('conv2d-320-columns', 2, 8, 8, 64, 64, 320, rpv='W', opts=dict(gemm_pp=0)),
        wcase('conv2d-320-columns', 2, 8, 8, 64, 64, 320, rpv='W', opts=dict(gemm_pp=1)),
    ]


def refusal_cases():
    """each one step outside the supported set: (name, the supported case it starts from, descriptor fields overwritten, answer).
    The buffers are those of the supported case, which is never smaller than what the overwritten description names."""
    one = wcase('refusal-base', 1, 6, 8, 16, 0, 16, pad=8)
    two = wcase('refusal-base-two-sources', 1, 4, 6, 64, 128, 8)
    U = VSX_E_UNSUPPORTED
    return [
        ('refuse-odd-H', one, dict(H=5, M=5 * 8), U),
        ('refuse-odd-W', one, dict(W=7, M=6 * 7), U),
        ('refuse-C1-12', one, dict(C1=12, K=9 * 12), U),
        ('refuse-two-sources-C2-72', two, dict(C2=72, K=9 * 136), U),
        ('refuse-N-12', one, dict(N=12), U),
        ('refuse-ldc-N+4', one, dict(ldc=20), U),
        ('refuse-ldr-N+4', one, dict(ldr=20), U),
        ('refuse-alpha-half', one, dict(alpha=0.5), U),
        ('refuse-batch', one, dict(batch0=2), U),
        ('refuse-rows-per-vec-0-with-a-row-vector', one, dict(rows_per_vec=0), U),
        ('refuse-workspace-one-byte-short', one, dict(), VSX_E_WORKSPACE),
    ]


GEOMETRY_CASES, CHANNEL_CASES, EPILOGUE_CASES, ROUNDED_CASES = geometry_cases(), channel_cases(), epilogue_cases(), rounded_cases()
WRAPPER_CASES, REFUSALS = wrapper_cases(), refusal_cases()
ENTRY_CASES = GEOMETRY_CASES + CHANNEL_CASES + EPILOGUE_CASES + ROUNDED_CASES
BY_NAME = {c['name']: c for c in ENTRY_CASES + WRAPPER_CASES}
assert len(BY_NAME) == len(ENTRY_CASES) + len(WRAPPER_CASES), 'two cases share a name'


# ------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------
def nvec(c):
    return (c['M'] + c['rpv'] - 1) // c['rpv']


def make_inputs(c):
    """host tensors of a case, by its name: x [nimg, H, W, C1], x2 or None, weight [N, 3, 3, C], bias [N], rowvec [ceil(M / rpv), N],
    residual [M, N] (the last three whether or not the epilogue uses them: a case and its epilogue subsets share the rest)"""
    g = gc._gen(c['name'])
    nimg, Hh, Ww, C1, C2, N, M = c['nimg'], c['H'], c['W'], c['C1'], c['C2'], c['N'], c['M']
    C = C1 + C2
    if c['cls'] == 'E':
        ax, aw = c['amp']
        x, w = gc._ints(g, -ax, ax, nimg, Hh, Ww, C), gc._ints(g, -aw, aw, N, 3, 3, C)
        bias = gc._bias_e(g, N, False)
        rowvec, residual = gc._ints(g, -2047, 2047, nvec(c), N), gc._ints(g, -2047, 2047, M, N)
    else:
        seed = int(torch.randint(0, 2 ** 31 - 1, (1,), generator=g))
        base = make_case(nimg, Hh, Ww, C, 0, N, seed=seed)
        x, w, bias = base['x'], base['weight'], base['bias']
        rowvec = (torch.randn(nvec(c), N, generator=g) * 0.3).half()
        scale = 1.0
        if c['res_scale']:
            scale = c['res_scale'] * float(reference(dict(base, bias=torch.zeros(N).half())).pow(2).mean().sqrt())
        residual = (torch.randn(M, N, generator=g) * scale).half()
    return dict(x=x[..., :C1].contiguous(), x2=x[..., C1:].contiguous() if C2 else None, weight=w, bias=bias, rowvec=rowvec, residual=residual)


def _xcat(host):
    return host['x'] if host['x2'] is None else torch.cat([host['x'], host['x2']], -1)


def exact_stages(c, host):
    """V, U, Mt of Inputs E in fp64, each asserted unchanged by a round trip through fp16; the epilogue's partial sums below 2^24"""
    x, w = _xcat(host).double(), host['weight'].double()
    d = F.pad(x, (0, 0, 1, 1, 1, 1)).unfold(1, 4, 2).unfold(2, 4, 2)
    v = torch.einsum('ar,nijcrs,bs->abnijc', BT.double(), d, BT.double()).reshape(16, -1, x.shape[-1])
    u = torch.einsum('ar,orsc,bs->aboc', G.double(), w, G.double()).reshape(16, w.shape[0], w.shape[3])
    mt = torch.bmm(v, u.transpose(1, 2))
    for name, t in (('V', v), ('U', u), ('Mt', mt)):
        assert bool((t.half().double() == t).all()), (c['name'], f'{name} is not fp16-exact: max |{name}| = {float(t.abs().max())}; lower the amplitude')
    conv = reference(dict(x=_xcat(host), x2=None, weight=host['weight'], bias=torch.zeros(c['N']).half(), rowvec=None, residual=None))
    worst = float(conv.abs().max()) + 4094 + 2047 + 2047
    assert worst < 2 ** 24, (c['name'], worst)
    return v, u, mt


class Problem:
    """the tensors of a case on `device` (kept alive here), their host copies, and the descriptor"""


def build(c, device, impl, over=None):
    """the descriptor of `c` with C and the workspace inside sentinel-filled buffers.  over: descriptor fields overwritten last
    (the refusals)"""
    pb = Problem()
    pb.c, pb.host, pb.dev = c, make_inputs(c), {}
    nimg, Hh, Ww, C1, C2, N, M, pad, epi = c['nimg'], c['H'], c['W'], c['C1'], c['C2'], c['N'], c['M'], c['pad'], c['epi']
    d = pb.d = impl.GemmDesc()
    d.M, d.N, d.K, d.batch0, d.batch1, d.alpha = M, N, 9 * (C1 + C2), 1, 1, 1.0
    d.a_mode, d.H, d.W, d.C1, d.C2, d.ks, d.stride = 1, Hh, Ww, C1, C2, 3, 1
    if c['pad11']:
        d.pad_lo = d.pad_hi = 1

    def put(name, t):
        pb.dev[name] = t.contiguous().to(device)
        return pb.dev[name].data_ptr()

    d.A = put('x', pb.host['x'])
    if C2:
        d.A2 = put('x2', pb.host['x2'])
    d.B, d.ldb = put('weight', pb.host['weight']), d.K          # the direct form reads it; the Winograd form must not
    pb.dev['u'] = impl.winograd_weights(pb.dev['weight'])
    pb.host['u'] = pb.dev['u'].cpu()
    if 'b' in epi:
        d.bias = put('bias', pb.host['bias'])
    if 'v' in epi:
        d.rowvec, d.rows_per_vec = put('rowvec', pb.host['rowvec']), c['rpv']
    ldc, ldr = N + pad, N + RPAD[pad]
    if 'r' in epi:
        rows = torch.full((M, ldr), gc.PAD_VALUE, dtype=H16)
        rows[:, :N] = pb.host['residual']
        d.residual, d.ldr = put('residual', rows), ldr
    # C: C_GUARD_ROWS sentinel rows in front and behind, and ldc - N sentinel columns behind every row
    coff = C_GUARD_ROWS * ldc
    pb.cidx = coff + torch.arange(M)[:, None] * ldc + torch.arange(N)[None, :]
    pb.cbuf = torch.full((coff + M * ldc + coff,), SENTINEL, dtype=H16).to(device)
    d.C, d.ldc = pb.cbuf.data_ptr() + 2 * coff, ldc
    # the workspace: exactly the bytes the formula of include/vsx.h gives, WS_GUARD sentinel elements on either side
    pb.ws_elems = 16 * (M // 4) * (C1 + C2 + N)
    pb.wsbuf = torch.full((WS_GUARD + pb.ws_elems + WS_GUARD,), SENTINEL, dtype=H16).to(device)
    pb.ws_ptr = pb.wsbuf.data_ptr() + 2 * WS_GUARD
    for k, v in (over or {}).items():
        setattr(d, k, v)
    return pb


def snapshot(pb):
    """host copies of everything the call can reach: C's buffer, the workspace's buffer and every input"""
    return dict(cbuf=pb.cbuf.cpu().clone(), wsbuf=pb.wsbuf.cpu().clone(), **{k: v.cpu().clone() for k, v in pb.dev.items()})


# ------------------------------------------------------------------------------------------------
# references
# ------------------------------------------------------------------------------------------------
def input_transform_ordered(x):
    """x fp16 [nimg, H, W, C] -> V fp16 [16, tiles, C]: B^T d B in fp32 with the kernel's operations in the kernel's order (down the
    columns first, then along the rows; additions and subtractions only), one rounding"""
    d = F.pad(x.float(), (0, 0, 1, 1, 1, 1)).unfold(1, 4, 2).unfold(2, 4, 2)           # [nimg, H/2, W/2, C, 4 (rows), 4 (columns)]
    d0, d1, d2, d3 = d[..., 0, :], d[..., 1, :], d[..., 2, :], d[..., 3, :]
    v = []
    for t in (d0 - d2, d1 + d2, d2 - d1, d1 - d3):                                    # a = 0 .. 3, each [..., 4 (columns)]
        t0, t1, t2, t3 = t[..., 0], t[..., 1], t[..., 2], t[..., 3]
        v += [t0 - t2, t1 + t2, t2 - t1, t1 - t3]                                     # b = 0 .. 3: xi = 4 a + b
    return torch.stack(v, 0).reshape(16, -1, x.shape[-1]).half()


def output_transform_ordered(mt, nimg, Hh, Ww):
    """Mt fp16 [16, tiles, N] -> fp32 [nimg * H * W, N]: A^T Mt A with the kernel's operations in the kernel's order"""
    m = mt.float().reshape(4, 4, nimg, Hh // 2, Ww // 2, -1)                           # [a, b, image, ti, tj, n]
    down = ((m[0] + m[1]) + m[2], (m[1] - m[2]) - m[3])                               # p = 0, 1, each [b, image, ti, tj, n]
    y = torch.stack([torch.stack([(s[0] + s[1]) + s[2], (s[1] - s[2]) - s[3]], 0) for s in down], 0)      # [p, q, image, ti, tj, n]
    return y.permute(2, 3, 0, 4, 1, 5).reshape(nimg * Hh * Ww, -1)


def epilogue(pb, acc, absolute=False):
    """acc [M, N] (any float dtype) + bias, + row vector, + residual, in that order, in acc's dtype"""
    c, host, dt = pb.c, pb.host, acc.dtype
    ab = (lambda t: t.abs()) if absolute else (lambda t: t)
    if 'b' in c['epi']:
        acc = acc + ab(host['bias'].to(dt))[None, :]
    if 'v' in c['epi']:
        acc = acc + ab(host['rowvec'].to(dt))[torch.arange(c['M']) // c['rpv']]
    if 'r' in c['epi']:
        acc = acc + ab(host['residual'].to(dt))
    return acc


def convolution64(pb):
    """the 3x3 convolution of the host inputs in fp64: [M, N]"""
    x, w = _xcat(pb.host).double(), pb.host['weight'].double()
    return F.conv2d(x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), padding=1).permute(0, 2, 3, 1).reshape(pb.c['M'], pb.c['N'])


# ------------------------------------------------------------------------------------------------
# the rule and the runners
# ------------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(torch.int16)


def _mismatches(got, want):
    return int((_bits(got) != _bits(want)).sum())


def check_untouched(pb, before, after, result=True):
    """every byte outside the result and outside the workspace is what it was (result=False: inside them as well)"""
    c = pb.c
    outside = torch.ones(after['cbuf'].numel(), dtype=torch.bool)
    if result:
        outside[pb.cidx.reshape(-1)] = False
    moved = (_bits(after['cbuf']) != _bits(before['cbuf'])) & outside
    assert not bool(moved.any()), (c['name'], 'stored outside the result', int(moved.sum()), 'first at element',
                                   int(moved.nonzero()[0]) - int(pb.cidx.min()), 'from C')
    outside = torch.ones(after['wsbuf'].numel(), dtype=torch.bool)
    if result:
        outside[WS_GUARD:WS_GUARD + pb.ws_elems] = False
    moved = (_bits(after['wsbuf']) != _bits(before['wsbuf'])) & outside
    assert not bool(moved.any()), (c['name'], 'stored outside the workspace', int(moved.sum()), 'first at element',
                                   int(moved.nonzero()[0]) - WS_GUARD, 'from its start')
    for k in pb.dev:
        assert torch.equal(after[k].view(torch.int16) if after[k].dtype == H16 else after[k],
                           before[k].view(torch.int16) if before[k].dtype == H16 else before[k]), (c['name'], f'input {k} was written')


def check_u(pb, fig):
    c, w = pb.c, pb.host['weight'].double()
    u = pb.host['u']
    assert u.shape == (16, c['N'], c['C1'] + c['C2']) and u.dtype == H16, (c['name'], tuple(u.shape))
    want = torch.einsum('ar,orsc,bs->aboc', G.double(), w, G.double()).reshape(u.shape)
    if c['cls'] == 'E':
        fig['u_mismatches'] = _mismatches(u, want.half())
        assert fig['u_mismatches'] == 0, (c['name'], 'U', fig)
    else:
        terms = torch.einsum('ar,orsc,bs->aboc', G.double().abs(), w.abs(), G.double().abs()).reshape(u.shape)
        bound = tk.ulp16(want) / 2 + 9 * 2.0 ** -24 * terms
        fig['u_ratio'] = float(((u.double() - want).abs() / bound).max())
        assert fig['u_ratio'] <= 1.0, (c['name'], 'U', fig)


def run_case(impl, device, c):
    t0 = time.time()
    nimg, Hh, Ww, N, M, tiles = c['nimg'], c['H'], c['W'], c['N'], c['M'], c['tiles']
    C = c['C1'] + c['C2']
    E = c['cls'] == 'E'
    with options(impl, c['opts']):
        pb = build(c, device, impl)
        exact = exact_stages(c, pb.host) if E else None
        need = impl.wino_workspace(pb.d)
        assert need > 0, (c['name'], 'vsx_conv3x3_winograd_workspace: the library does not take this description')
        assert need == 2 * pb.ws_elems, (c['name'], need)
        before = snapshot(pb)
        outs = []
        for _ in range(2):
            rc = impl.winograd(pb.d, pb.dev['u'].data_ptr(), pb.ws_ptr, need)
            assert rc == VSX_OK, (c['name'], rc)
            impl.sync()
            outs.append(snapshot(pb))
        after = outs[0]
        direct = None
        if not E:                                   # the direct form of the same description, into a buffer of its own
            d2 = impl.GemmDesc.from_buffer_copy(pb.d)
            dbuf = torch.full_like(pb.cbuf, SENTINEL)
            d2.C = dbuf.data_ptr() + 2 * C_GUARD_ROWS * pb.d.ldc
            impl.gemm(d2)
            impl.sync()
            direct = dbuf.cpu()[pb.cidx]
    fig = dict(case=c['name'], cls=c['cls'], elements=M * N)
    check_u(pb, fig)
    ws = after['wsbuf'][WS_GUARD:WS_GUARD + pb.ws_elems]
    v, mt = ws[:16 * tiles * C].view(16, tiles, C), ws[16 * tiles * C:].view(16, tiles, N)
    y = after['cbuf'][pb.cidx]
    u = pb.host['u']
    # V: the kernel's arithmetic in the kernel's order, on the inputs
    fig['v_mismatches'] = _mismatches(v, input_transform_ordered(_xcat(pb.host)))
    # Y: the kernel's arithmetic in the kernel's order, on the kernel's own Mt
    fig['y_mismatches'] = _mismatches(y, epilogue(pb, output_transform_ordered(mt, nimg, Hh, Ww)).half())
    if E:
        v64, u64, mt64 = exact
        want = epilogue(pb, convolution64(pb))
        want16 = want.half()
        fig.update(v_mismatches_fp64=_mismatches(v, v64.half()), mt_mismatches=_mismatches(mt, mt64.half()),
                   y_mismatches_fp64=_mismatches(y, want16), ties=int(((want - want16.double()).abs() * 2 == tk.ulp16(want)).sum()))
        failed = [k for k in ('v_mismatches', 'v_mismatches_fp64', 'mt_mismatches', 'y_mismatches', 'y_mismatches_fp64') if fig[k]]
    else:
        # Mt: the batched GEMM on the kernel's own V and U, under gemm_case's rule
        want = torch.bmm(v.double(), u.double().transpose(1, 2))
        ideal = torch.bmm(v.float(), u.float().transpose(1, 2)).half()
        S = torch.bmm(v.double().abs(), u.double().abs().transpose(1, 2))
        extra = 2.0 ** -10 * want.pow(2).mean(-1, keepdim=True).sqrt() + (C + 4) * 2.0 ** -24 * S
        mfig, failed = measure(mt, want, ideal, extra)
        fig.update({'mt_' + k: val for k, val in mfig.items()})
        failed = ['mt_' + m for m in failed] + [k for k in ('v_mismatches', 'y_mismatches') if fig[k]]
        # end to end against the true convolution: the bounds of tests/test_winograd_gpu.py
        ref = epilogue(pb, convolution64(pb))
        fig.update(rel_l2=rel_l2(y, ref), rel_l2_direct=rel_l2(direct, ref), rel_l2_bound=REL_L2_BOUND, ratio_bound=RATIO_BOUND)
        fig['ratio_to_direct'] = fig['rel_l2'] / fig['rel_l2_direct']
        if not fig['rel_l2'] < REL_L2_BOUND:
            failed.append('rel_l2')
        if not fig['rel_l2'] <= RATIO_BOUND * fig['rel_l2_direct']:
            failed.append('ratio_to_direct')
    fig['repeat_mismatches'] = _mismatches(outs[0]['cbuf'], outs[1]['cbuf']) + _mismatches(outs[0]['wsbuf'], outs[1]['wsbuf'])
    if fig['repeat_mismatches']:
        failed.append('repeat_mismatches')
    fig['wall_seconds'] = time.time() - t0
    print(' '.join(f'{k}={val:.3e}' if isinstance(val, float) else f'{k}={val}' for k, val in fig.items()))
    FIGURES.append(fig)
    assert not failed, (c['name'], failed, fig)
    check_untouched(pb, before, after)
    return fig


def run_refusal(impl, device, r):
    """the library answers `status` and writes nothing: C's buffer, the workspace's buffer and every input are what they were"""
    name, c, over, status = r
    with options(impl, c['opts']):
        pb = build(c, device, impl, over)
        need = impl.wino_workspace(pb.d)
        if status == VSX_E_WORKSPACE:
            assert need == 2 * pb.ws_elems, (name, need)
            given = need - 1
        else:
            assert need == 0, (name, 'vsx_conv3x3_winograd_workspace takes it', need)
            given = 2 * pb.ws_elems
        before = snapshot(pb)
        rc = impl.winograd(pb.d, pb.dev['u'].data_ptr(), pb.ws_ptr, given)
        impl.sync()
        after = snapshot(pb)
    assert rc == status, (name, rc)
    check_untouched(pb, before, after, result=False)


def run_wrapper(impl, device, c):
    """ops.conv2d under conv_winograd = 2 on Inputs E: the Winograd launch ran, once, and the bits are the fp64 result rounded once"""
    t0 = time.time()
    with options(impl, c['opts']):
        pb = Problem()
        pb.c, pb.host = c, make_inputs(c)
        exact_stages(c, pb.host)
        dev = {k: (t.to(device) if t is not None else None) for k, t in pb.host.items()}
        y, launches = impl.conv2d(dev['x'], dev['weight'], dev['bias'] if 'b' in c['epi'] else None, x2=dev['x2'],
                                  rowvec=dev['rowvec'] if 'v' in c['epi'] else None, rows_per_vec=c['rpv'] if 'v' in c['epi'] else 0,
                                  residual=dev['residual'].view(c['nimg'], c['H'], c['W'], c['N']) if 'r' in c['epi'] else None)
        impl.sync()
        family = impl.batched_family(c)
    assert launches == 1, (c['name'], 'Winograd launches', launches)
    want = epilogue(pb, convolution64(pb))
    want16 = want.half()
    fig = dict(case=c['name'], cls='E', elements=want.numel(), y_mismatches_fp64=_mismatches(y.cpu().reshape(want.shape), want16),
               ties=int(((want - want16.double()).abs() * 2 == tk.ulp16(want)).sum()), gemm_family=family, wall_seconds=time.time() - t0)
    FIGURES.append(fig)
    assert fig['y_mismatches_fp64'] == 0, (c['name'], fig)
    return fig


def batched_desc(impl, c):
    """the batched description the entry point hands to vsx_gemm_f16 (csrc/winograd.hip), for the plan query"""
    g = impl.GemmDesc()
    C, tiles = c['C1'] + c['C2'], c['tiles']
    g.M, g.N, g.K, g.batch0, g.batch1, g.alpha = tiles, c['N'], C, 16, 1, 1.0
    g.A = g.B = g.C = 0x10000
    g.lda, g.a_bs0, g.ldb, g.b_bs0, g.ldc, g.c_bs0 = C, tiles * C, C, c['N'] * C, c['N'], tiles * c['N']
    return g


def expected_figures():
    return len(ENTRY_CASES) + len(WRAPPER_CASES)


# ------------------------------------------------------------------------------------------------
# one large-index case, checked on a sample of tiles
# ------------------------------------------------------------------------------------------------
# M (C1 + C2) = 2^31 - 2^20, one step of W below the limit of the form: V has 4 M C = 2^33 - 2^22 elements, so 16 tiles C, every
# xi plane offset k * tiles * C from k = 4 and the batched GEMM's z * a_bs0 pass 2^31 elements (and 2^32 bytes from k = 1).
# 4.3 GB of input, 18.2 GB of workspace.
LARGE = dict(nimg=2, H=2048, W=4094, C=128, N=8)
SMALL_STAND_IN = dict(nimg=2, H=4, W=6, C=8, N=8)            # the same code path on the CPU (tests/test_winograd_case.py)


def large_sample(shape, nrandom=64):
    """tile indices: the first, the last, the four corners of the last image, and `nrandom` pseudo-random ones"""
    nimg, th, tw = shape['nimg'], shape['H'] // 2, shape['W'] // 2
    tiles, last = nimg * th * tw, (nimg - 1) * th * tw
    fixed = [0, tiles - 1, last, last + tw - 1, last + (th - 1) * tw, last + th * tw - 1]
    rnd = torch.randint(0, tiles, (nrandom,), generator=torch.Generator().manual_seed(20251)).tolist()
    return torch.tensor(sorted(set(fixed + rnd)))


def run_large(impl, device, shape=LARGE):
    """Inputs E generated on the device; V, Mt and Y of the sampled tiles bit-equal to fp64 computed from their input windows alone"""
    t0 = time.time()
    nimg, Hh, Ww, C, N = shape['nimg'], shape['H'], shape['W'], shape['C'], shape['N']
    M, th, tw = nimg * Hh * Ww, Hh // 2, Ww // 2
    tiles = M // 4
    name = f'large-index-E-{nimg}x{Hh}x{Ww}-{C}+0-to{N}-bvr'
    g = gc._gen(name)
    dg = torch.Generator(device=device).manual_seed(7)
    x = torch.randint(-3, 4, (nimg, Hh, Ww, C), generator=dg, device=device, dtype=torch.int8).to(H16)
    ldc, ldr = N, N + 8
    res = torch.randint(-2047, 2048, (M, ldr), generator=dg, device=device, dtype=torch.int16).to(H16)
    host = dict(weight=gc._ints(g, -2, 2, N, 3, 3, C), bias=gc._bias_e(g, N, False), rowvec=gc._ints(g, -2047, 2047, nimg, N))
    dev = {k: t.to(device) for k, t in host.items()}
    u = impl.winograd_weights(dev['weight'])
    d = impl.GemmDesc()
    d.M, d.N, d.K, d.batch0, d.batch1, d.alpha = M, N, 9 * C, 1, 1, 1.0
    d.a_mode, d.H, d.W, d.C1, d.C2, d.ks, d.stride = 1, Hh, Ww, C, 0, 3, 1
    d.A, d.B, d.ldb = x.data_ptr(), dev['weight'].data_ptr(), d.K
    d.bias, d.rowvec, d.rows_per_vec, d.residual, d.ldr = dev['bias'].data_ptr(), dev['rowvec'].data_ptr(), Hh * Ww, res.data_ptr(), ldr
    coff = C_GUARD_ROWS * ldc
    cbuf = torch.full((coff + M * ldc + coff,), SENTINEL, dtype=H16, device=device)
    d.C, d.ldc = cbuf.data_ptr() + 2 * coff, ldc
    ws_elems = 16 * tiles * (C + N)
    wsbuf = torch.empty(WS_GUARD + ws_elems + WS_GUARD, dtype=H16, device=device)      # (the call writes every element between the guards)
    wsbuf[:WS_GUARD] = SENTINEL
    wsbuf[WS_GUARD + ws_elems:] = SENTINEL
    with options(impl, {}):
        need = impl.wino_workspace(d)
        assert need > 0, (name, 'vsx_conv3x3_winograd_workspace: the library does not take this description')
        assert need == 2 * ws_elems and M * C < 2 ** 31, (name, need)
        impl.sync()
        t1 = time.time()
        rc = impl.winograd(d, u.data_ptr(), wsbuf.data_ptr() + 2 * WS_GUARD, need)
        assert rc == VSX_OK, (name, rc)
        impl.sync()
        t2 = time.time()
    # what the call left for the sampled tiles
    s = large_sample(shape)
    sd = s.to(device)
    def planes(first, width):                   # [16, S, width], one xi plane (fewer than 2^31 elements) at a time
        return torch.stack([wsbuf[first + k * tiles * width:first + (k + 1) * tiles * width].view(tiles, width)[sd] for k in range(16)]).cpu()
    V, Mt = planes(WS_GUARD, C), planes(WS_GUARD + 16 * tiles * C, N)
    img, r = s // (th * tw), s % (th * tw)
    ti, tj = r // tw, r % tw
    pq = torch.arange(2)
    rows = ((img[:, None, None] * Hh + 2 * ti[:, None, None] + pq[None, :, None]) * Ww + 2 * tj[:, None, None] + pq[None, None, :])   # [S, 2, 2]
    Y = cbuf[coff:coff + M * ldc].view(M, ldc)[rows.to(device)].cpu()                                 # [S, 2, 2, N]
    # the fp64 reference from the 4 x 4 input windows of those tiles alone
    y = 2 * ti[:, None] - 1 + torch.arange(4)[None, :]
    xx = 2 * tj[:, None] - 1 + torch.arange(4)[None, :]
    inside = ((y >= 0) & (y < Hh))[:, :, None] & ((xx >= 0) & (xx < Ww))[:, None, :]
    pix = (img[:, None, None] * Hh + y.clamp(0, Hh - 1)[:, :, None]) * Ww + xx.clamp(0, Ww - 1)[:, None, :]
    win = x.view(M, C)[pix.to(device)].cpu().double()                                                # [S, 4, 4, C]
    win[~inside] = 0
    w64 = host['weight'].double()
    v64 = torch.einsum('ar,trsc,bs->abtc', BT.double(), win, BT.double()).reshape(16, len(s), C)
    u64 = torch.einsum('ar,orsc,bs->aboc', G.double(), w64, G.double()).reshape(16, N, C)
    mt64 = torch.bmm(v64, u64.transpose(1, 2))
    for nm, t in (('V', v64), ('U', u64), ('Mt', mt64)):
        assert bool((t.half().double() == t).all()), (name, f'{nm} of a sampled tile is not fp16-exact')
    conv = torch.stack([torch.stack([torch.einsum('orsc,trsc->to', w64, win[:, p:p + 3, q:q + 3]) for q in (0, 1)], 1) for p in (0, 1)], 1)   # [S, 2, 2, N]
    want = conv + host['bias'].double() + host['rowvec'].double()[img][:, None, None, :] + res[rows.to(device)][..., :N].cpu().double()
    fig = dict(case=name, cls='E', elements=want.numel(), sampled_tiles=len(s), v_elements_total=16 * tiles * C,
               u_mismatches=_mismatches(u.cpu(), u64.half()), v_mismatches_fp64=_mismatches(V, v64.half()),
               mt_mismatches=_mismatches(Mt, mt64.half()), y_mismatches_fp64=_mismatches(Y, want.half()),
               ties=int(((want - want.half().double()).abs() * 2 == tk.ulp16(want)).sum()))
    guards = torch.cat([cbuf[:coff], cbuf[coff + M * ldc:], wsbuf[:WS_GUARD], wsbuf[WS_GUARD + ws_elems:]]).cpu()
    fig['guard_elements_moved'] = int((guards != SENTINEL).sum())
    fig.update(launch_seconds=t2 - t1, wall_seconds=time.time() - t0)
    print(' '.join(f'{k}={val:.3e}' if isinstance(val, float) else f'{k}={val}' for k, val in fig.items()))
    FIGURES.append(fig)
    failed = [k for k in ('u_mismatches', 'v_mismatches_fp64', 'mt_mismatches', 'y_mismatches_fp64', 'guard_elements_moved') if fig[k]]
    assert not failed, (name, failed, fig)
    return fig

