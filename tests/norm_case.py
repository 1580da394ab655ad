"""Shared by tests/test_norm_kernels_gpu.py (the HIP kernels of videoswap_amd/csrc/norm.hip and the scalar glue of
csrc/elementwise.hip) and tests/test_norm_case.py (CPU stand-ins and deliberate mutants of them): case tables, fp64 references
on fp16-exact inputs in plain PyTorch, and the comparison rule.  No kernels and no GPU calls of its own: every runner takes the
function under test and a device.  The rule itself (`measure`, `ulp16`) is tests/train_kernel_case.py's, imported, not copied.

Two references per op, each written as TWO-PASS (mean, then the centred variance) and taking a dtype: `want` is the float64
result, `ideal` the float32 result rounded to fp16.  The kernels whose form is ONE-PASS by design (gn_stats_kernel +
gn_finalize_kernel / gn_mean_rstd, row_stats_combine_kernel: var = max(fma(-mean, mean, q / n), 0) from fp32 sums of x and x^2)
get a second, FORM ideal: the same statement in fp32, rounded to fp16.

    two-pass kernels (vsx_layernorm, vsx_row_stats)      the unchanged rule against the two-pass ideal, at every rung
    one-pass kernels (GroupNorm forward, vsx_row_stats_combine)
                                                         the unchanged rule with every metric of the ideal replaced by
                                                         two-pass ideal + SPREAD x max(form ideal - two-pass ideal, 0)
    the folded LayerNorm (ops.DeferredLN)                the unchanged rule against the two-pass ideal, except in the cases named
                                                         in FOLD_FORM_RUNGS, where the float32 restatement of the fold's algebraic
                                                         form itself misses that rule: those take the replacement above

That replacement is never wider than max(two-pass ideal, SPREAD x form ideal) and meets it where the one-pass error dominates.
Where it does not (the base rung, every edge shape: form ideal = two-pass ideal, both made of the fp16 output rounding) it IS the
two-pass rule: SPREAD, measured where the one-pass error dominates, is 3.5 to 5.6 for GroupNorm, and a plain maximum would widen
every bound by that factor on inputs at which the summation order changes nothing (under it the mutants `n_minus_1` and
`fp16_stats` of tests/test_norm_case.py pass at 2 x 100 x 320 on the base rung).  The form ideal's error is the output rounding
plus one rounding of the statistics; only the second depends on the order, so only the excess over the two-pass ideal is scaled.
The per-element bound, which the rule states absolutely (1 = one fp16 ulp + 2^-10 row rms), becomes
min(1 + SPREAD x excess of the form ideal's ratio, max(1, SPREAD x the form ideal's ratio)).  The fp32 statistics have no output
rounding to hide the order behind, their SPREAD holds at every rung, and they take the plain maximum.

The one-pass error is one random rounding per group (or row) whose size depends on the summation order.  SPREAD is the largest
ratio, per metric, between any two of five summation orders of the form ideal over the shift ladder: measured on the references
alone (`measure_spread`, recomputed and asserted by tests/test_norm_case.py), written down below, never tuned to a kernel.  So
the rule allows another order and nothing more.

fp32 statistics (rstd, -rstd * mean): the relative error of rstd and the absolute error of -rstd * mean over 1 + |want| must
stay within 4 x the float32 restatement's worst value + 2^-22.  2^-22: v_rsq_f32 is good to one ulp (2^-23 relative), the
multiply by the mean and the store of the product round once more (2^-24 each), and twice that sum is room, not tuning.
"""
import torch
import torch.nn.functional as F

import train_kernel_case as tk
from train_kernel_case import H, _gen, measure, ulp16      # noqa: F401  (ulp16: re-exported for the tests)

EPS = 1e-5
FIGURES = []                    # one dict per compared tensor
METRICS = ('l2', 'row', 'maxabs', 'elem')
FACTOR = {'l2': 1.5, 'row': 2.0, 'maxabs': 4.0}
STAT_ROOM = 2.0 ** -22
RULE = ('against fp64; ideal = the two-pass fp32 reference rounded to fp16: l2 <= 1.5 ideal, worst row <= 2 ideal, max-abs <= 4 '
        'ideal, per element <= 1 fp16 ulp + 2^-10 row rms (elem_* are ratios to that bound).  One-pass kernels, and the folded '
        'LayerNorm where its form itself misses that rule (asserted = form): every ideal metric replaced by two-pass ideal + spread x max(form ideal - two-pass ideal, 0) (never wider than '
        'max(two-pass ideal, spread x form ideal)), elem bound min(1 + spread x excess, max(1, spread x form)).  fp32 '
        'statistics: rel err of rstd and |err| / (1 + |want|) of -rstd mean <= 4 x the fp32 restatement (one-pass: max(two-pass, '
        'spread x form)) + 2^-22')

# Largest ratio between two summation orders (ORDERS) of the form ideal, per metric, over the ladder: `measure_spread` of this
# file on the references alone, rounded up to two digits.  tests/test_norm_case.py recomputes it and asserts it is not exceeded
# (SPREAD_HOST_TOL there: 'whole' and the chunk sums go through torch.sum / matmul, whose own order follows the vector width and the
# thread count of the host).
SPREAD = {
    'group_norm': {'l2': 5.7, 'row': 5.2, 'maxabs': 3.6, 'elem': 3.5},           # measured 5.62, 5.11, 3.54, 3.47
    'row_stats_combine': {'rstd': 4.2, 'shift': 4.2},                            # measured 4.12, 4.13
    'folded': {'l2': 1.1, 'row': 1.1, 'maxabs': 1.1, 'elem': 1.3},               # measured 1.05, 1.07, 1.01, 1.22
}

# the shift ladder: (name, kind, scale, shift, mean / std of the input)
LADDER = [('randn*1.5+0.3', 'randn', 1.5, 0.3, 0.2), ('randn+8', 'randn', 1.0, 8.0, 8.0), ('randn+32', 'randn', 1.0, 32.0, 32.0),
          ('uniform*0.5+8', 'uniform', 0.5, 8.0, 57.2), ('uniform*0.5+16', 'uniform', 0.5, 16.0, 112.6),
          ('uniform*0.5+32', 'uniform', 0.5, 32.0, 223.4), ('randn+64', 'randn', 1.0, 64.0, 64.0)]
RUNGS = range(len(LADDER))
# beside the ladder: activations whose variance (1.5e-5) is that of eps, so that the place and the size of eps show
TINY = ('randn*2^-8', 'randn', 2.0 ** -8, 0.0, 0.0)


def rung_of(rung):
    return TINY if rung == 'tiny' else LADDER[rung]


def _rid(rung):
    """a ladder rung as the figures carry it: the base rung and everything beside the ladder count as rung 0 / no rung"""
    return rung if isinstance(rung, int) else None


def _rtag(rung):
    return '' if rung == 0 else '-' + rung_of(rung)[0]


def rung_tensor(g, rung, *shape):
    _, kind, scale, shift, _ = rung_of(rung)
    t = torch.randn(*shape, generator=g) if kind == 'randn' else torch.rand(*shape, generator=g)
    return (t * scale + shift).to(H)


def _randn(g, *shape, scale=1.0, shift=0.0):
    return (torch.randn(*shape, generator=g) * scale + shift).to(H)


def _show(fig):
    print(' '.join(f'{k}={v:.3e}' if isinstance(v, float) else f'{k}={v}' for k, v in fig.items()))


# ------------------------------------------------------------------------------------------------
# the rule, bound to this file's FIGURES
# ------------------------------------------------------------------------------------------------
def check(name, got, want, ideal, kernel=None, rung=None, elem_extra=None):
    """train_kernel_case.check (the unchanged rule), its figure moved into this file's FIGURES"""
    n = len(tk.FIGURES)
    try:
        fig = tk.check(name, got, want, ideal, elem_extra)
        tk.FIGURES[-1].update(kernel=kernel, rung=rung, two_pass_rule=True)
        return fig
    finally:
        if len(tk.FIGURES) > n and 'two_pass_rule' not in tk.FIGURES[-1]:
            tk.FIGURES[-1].update(kernel=kernel, rung=rung, two_pass_rule=False)
        FIGURES.extend(tk.FIGURES[n:])
        del tk.FIGURES[n:]


def check_form(name, got, want, ideal, form, spread, kernel=None, rung=None, use_form=True):
    """the rule of the one-pass kernels: figures against BOTH ideals, bounds from two-pass ideal + spread x its excess.
    use_form=False: the same figures are recorded, but the bounds asserted are the unchanged two-pass rule's"""
    fig, failed2 = measure(got, want, ideal)
    ffig, _ = measure(form, want, ideal)
    fig = dict(case=name, kernel=kernel, rung=rung, **fig)
    failed = []
    for m in METRICS:
        fig[m + '_form'] = ffig[m + '_kernel']
        fig[m + '_two_pass_bound'] = fig[m + '_bound']
        excess = spread[m] * max(fig[m + '_form'] - fig[m + '_ideal'], 0.0) if use_form else 0.0
        fig[m + '_form_two_pass_ratio'] = fig[m + '_form'] / max(fig[m + '_two_pass_bound'], 1e-300)
        if not use_form:
            pass
        elif m == 'elem':
            fig[m + '_bound'] = min(1.0 + excess, max(1.0, spread[m] * fig[m + '_form']))
        else:
            fig[m + '_bound'] = FACTOR[m] * (fig[m + '_ideal'] + excess)
        if not fig[m + '_kernel'] <= fig[m + '_bound']:
            failed.append(m)
    if not fig['finite']:
        failed.append('finite')
    fig['two_pass_rule'], fig['asserted'] = not failed2, 'form' if use_form else 'two_pass'
    _show(fig)
    FIGURES.append(fig)
    assert not failed, (name, failed, fig)
    return fig


def _stat_err(t, want):
    t = t.double()
    return float((t[:, 0] / want[:, 0] - 1).abs().max()), float(((t[:, 1] - want[:, 1]).abs() / (1 + want[:, 1].abs())).max())


def check_stats(name, got, want, rest, form=None, spread=None, kernel=None, rung=None):
    """[M, 2] fp32 (rstd, -rstd * mean) against fp64; `rest` the two-pass float32 restatement, `form` the one-pass one"""
    assert got.dtype == torch.float32 and got.shape == want.shape and want.dtype == torch.float64, (got.dtype, tuple(got.shape))
    fig = {'case': name, 'kernel': kernel, 'rung': rung, 'finite': bool(torch.isfinite(got).all())}
    failed = []
    for i, m in enumerate(('rstd', 'shift')):
        fig[m + '_ideal'], fig[m + '_kernel'] = _stat_err(rest, want)[i], _stat_err(got, want)[i]
        base = fig[m + '_ideal']
        fig[m + '_two_pass_bound'] = 4 * base + STAT_ROOM
        if form is not None:
            fig[m + '_form'] = _stat_err(form, want)[i]
            base = max(base, spread[m] * fig[m + '_form'])
        fig[m + '_bound'] = 4 * base + STAT_ROOM
        if not fig[m + '_kernel'] <= fig[m + '_bound']:
            failed.append(m)
    fig['two_pass_rule'] = all(fig[m + '_kernel'] <= fig[m + '_two_pass_bound'] for m in ('rstd', 'shift'))
    if not fig['finite']:
        failed.append('finite')
    _show(fig)
    FIGURES.append(fig)
    assert not failed, (name, failed, fig)
    return fig


def envelopes(figures=None):
    """per kernel: the ladder rungs at which it met the plain TWO-PASS rule, and the envelope, the largest mean / std of the
    input up to which it met that rule at every rung (rungs taken in order of mean / std)"""
    out = {}
    for fig in (FIGURES if figures is None else figures):
        if fig.get('rung') is None or fig.get('kernel') is None:
            continue
        k = out.setdefault(fig['kernel'], {})
        k[fig['rung']] = k.get(fig['rung'], True) and bool(fig['two_pass_rule'])
    res = {}
    for kernel, rungs in out.items():
        env = None
        for r in sorted(rungs, key=lambda r: LADDER[r][4]):
            if not rungs[r]:
                break
            env = r
        res[kernel] = {'meets_two_pass_rule': {LADDER[r][0]: ok for r, ok in sorted(rungs.items())},
                       'envelope_rung': None if env is None else LADDER[env][0],
                       'envelope_mean_over_std': None if env is None else LADDER[env][4]}
    return res


# ------------------------------------------------------------------------------------------------
# references.  Two-pass, in `dt` (float64: want; float32, rounded to fp16: ideal)
# ------------------------------------------------------------------------------------------------
def ref_group_norm(x, x2, gamma, beta, groups, eps, nimg, silu, dt, count_rows=None):
    """[nimg, rows, C1 (+ C2)].  count_rows: the statistics are those of count_rows rows of which x holds `rows`
    (sum (x - mean)^2 / n + (1 - m / n) mean^2 is q / n - mean^2 with the sums taken over the m elements present)"""
    xin = (x if x2 is None else torch.cat([x, x2], dim=-1)).to(dt)
    C = xin.shape[-1]
    cpg = C // groups
    xs = xin.reshape(nimg, -1, groups, cpg)
    rows = xs.shape[1]
    n = float((rows if count_rows is None else count_rows) * cpg)
    mean = xs.sum((1, 3), keepdim=True) / n
    d = xs - mean
    var = (d * d).sum((1, 3), keepdim=True) / n
    if count_rows is not None and count_rows != rows:
        var = var + (1.0 - rows * cpg / n) * mean * mean
    y = (d * (var + eps).rsqrt()).reshape(nimg, rows, C) * gamma.to(dt) + beta.to(dt)
    return y * torch.sigmoid(y) if silu else y


def _pe_rows(pe, M, rows_per_frame, frames, frame_offset, dt):
    idx = (torch.arange(M, device=pe.device) // rows_per_frame) % frames + frame_offset
    return pe.to(dt)[idx]


def ref_layer_norm(x, gamma, beta, eps, dt, pe=None, rows_per_frame=0, frames=0, frame_offset=0):
    xf = x.to(dt)
    mean = xf.mean(-1, keepdim=True)
    d = xf - mean
    y = d * ((d * d).mean(-1, keepdim=True) + eps).rsqrt() * gamma.to(dt) + beta.to(dt)
    if pe is not None:
        y = y + _pe_rows(pe, x.shape[0], rows_per_frame, frames, frame_offset, dt)
    return y


def ref_row_stats(x, eps, dt):
    xf = x.to(dt)
    mean = xf.mean(-1)
    d = xf - mean[:, None]
    rstd = ((d * d).mean(-1) + eps).rsqrt()
    return torch.stack([rstd, -rstd * mean], dim=-1)


def _gelu(g):
    return g * 0.5 * torch.erfc(-g * 0.7071067811865476)


def ref_ln_linear(x, gamma, beta, eps, w, b, dt, pe=None, rows_per_frame=0, frames=0, frame_offset=0, residual=None, geglu=False):
    y = ref_layer_norm(x, gamma, beta, eps, dt, pe, rows_per_frame, frames, frame_offset) @ w.to(dt).t() + b.to(dt)
    if geglu:
        h, g = y.chunk(2, dim=-1)
        y = h * _gelu(g)
    return y if residual is None else y + residual.to(dt)


# ------------------------------------------------------------------------------------------------
# form ideals: the one-pass statement in fp32 under a choice of summation order
# ------------------------------------------------------------------------------------------------
ORDERS = ('whole', 'chunk8', 'chunk64', 'chunk512', 'serial')


def _one_pass(s, q, inv_n, eps):
    """fp32 (sum, sum of squares) -> (mean, rstd): mean = s / n, var = max(fma(-mean, mean, q / n), 0).  The fma is taken in
    double (the product of two floats is exact there) and rounded to float once"""
    mean = s * inv_n
    var = ((q * inv_n).double() - mean.double() * mean.double()).float().clamp_min(0)
    return mean, (var + eps).rsqrt()


def _serial(t, dim):
    """a running fp32 sum along `dim`, one element after the other: the last entry of a float32 cumsum"""
    acc = torch.zeros_like(t.select(dim, 0))
    for i in range(t.shape[dim]):
        acc = acc + t.select(dim, i)
    return acc


def _chunked(t, dim, r):
    """sums of `r` consecutive elements along `dim`, then the sum of those"""
    t = t.movedim(dim, -1)
    n = t.shape[-1]
    nch = -(-n // r)
    t = F.pad(t, (0, nch * r - n))
    return t.reshape(*t.shape[:-1], nch, r).sum(-1).sum(-1)


def gn_sums(xs, order):
    """xs [nimg, rows, groups, cpg] fp32 -> [nimg, groups]: rows in the given order, then the channels of the group"""
    if order == 'whole':
        return xs.sum((1, 3))
    if order == 'serial':
        return _serial(_serial(xs, 1), -1)
    return _chunked(xs, 1, int(order[5:])).sum(-1)


def form_group_norm(x, x2, gamma, beta, groups, eps, nimg, silu, order='whole'):
    xin = (x if x2 is None else torch.cat([x, x2], dim=-1)).float()
    C = xin.shape[-1]
    cpg = C // groups
    xs = xin.reshape(nimg, -1, groups, cpg)
    inv_n = torch.tensor(1.0 / (xs.shape[1] * cpg), dtype=torch.float32, device=xin.device)
    mean, rstd = _one_pass(gn_sums(xs, order), gn_sums(xs * xs, order), inv_n, eps)
    y = ((xs - mean[:, None, :, None]) * rstd[:, None, :, None]).reshape(xin.shape) * gamma.float() + beta.float()
    return (y * torch.sigmoid(y) if silu else y).to(H)


def row_sums(t, order):
    """t [M, C] fp32 -> [M]"""
    if order == 'whole':
        return t.sum(-1)
    if order == 'serial':
        return _serial(t, -1)
    return _chunked(t, -1, int(order[5:]))


def form_row_stats(x, eps, order='whole'):
    xf = x.float()
    inv_c = torch.tensor(1.0 / x.shape[-1], dtype=torch.float32, device=x.device)
    mean, rstd = _one_pass(row_sums(xf, order), row_sums(xf * xf, order), inv_c, eps)
    return torch.stack([rstd, -rstd * mean], dim=-1)


def fold_matmul(xf, wf, order):
    """xf [M, K] @ wf[N, K]^T in fp32 with the K axis summed in the given order"""
    if order == 'whole':
        return xf @ wf.t()
    if order == 'serial':
        acc = torch.zeros(xf.shape[0], wf.shape[0], dtype=torch.float32, device=xf.device)
        for k in range(xf.shape[1]):
            acc = acc + xf[:, k, None] * wf[None, :, k]
        return acc
    r = int(order[5:])
    acc = None
    for k0 in range(0, xf.shape[1], r):
        part = xf[:, k0:k0 + r] @ wf[:, k0:k0 + r].t()
        acc = part if acc is None else acc + part
    return acc


def form_ln_linear(x, gamma, beta, eps, w, b, pe=None, rows_per_frame=0, frames=0, frame_offset=0, residual=None, geglu=False,
                   order='whole'):
    """the algebraic form of the fold (ops.DeferredLN) in fp32 with its fp16 operands:
    rstd (x W'^T) - rstd mean sum_k W' + c2 (+ the fp16 rows pe W^T), W' = fp16(W o gamma), c2 = fp16(beta W^T + b)"""
    w32 = w.float()
    wf = (w32 * gamma.float()[None, :]).to(H).float()
    c1 = wf.sum(1)
    c2 = (w32 @ beta.float() + b.float()).to(H).float()
    st = ref_row_stats(x, eps, torch.float32)
    y = st[:, :1] * fold_matmul(x.float(), wf, order) + st[:, 1:] * c1[None, :] + c2[None, :]
    if pe is not None:
        rv = (pe.float() @ w32.t()).to(H)
        y = y + _pe_rows(rv, x.shape[0], rows_per_frame, frames, frame_offset, torch.float32)
    if geglu:
        h, g = y.chunk(2, dim=-1)
        y = h * _gelu(g)
    if residual is not None:
        y = y + residual.float()
    return y.to(H)


# ------------------------------------------------------------------------------------------------
# GroupNorm forward.  (nimg, rows, C1, C2, groups): the path each case reaches is named beside it
# ------------------------------------------------------------------------------------------------
GN_LADDER = (2, 100, 320, 0, 32)
GN_HUGE = (1, 2 ** 20 + 37, 8, 0, 2)
GN_ZERO = (2, 33, 96, 0, 8)               # + a group of zeros: image 1, group 5 (cpg 12: its channels start inside a vector)
GN_CASES = [
    (3, 50, 64, 0, 32),                   # ragged chunk
    GN_LADDER,                            # cpg 10: a 16-byte vector straddles groups
    (2, 77, 640, 320, 32),                # concat, cpg 30
    (1, 9, 1280, 1280, 32),               # rp = 1
    (1, 17, 4096, 0, 32),                 # both LDS arrays full
    (2, 33, 64, 0, 64),                   # cpg 1: eight groups inside one vector (the `left == 0` walk of the apply kernel)
    GN_ZERO,                              # cpg 12
    (2, 33, 32, 0, 1),                    # one group
    (1, 5, 8, 0, 1), (4, 1, 8, 0, 2),     # fewer rows than a chunk; C = 8 (512 rows per pass)
    (2, 41, 520, 0, 8),                   # 65 vectors per row: 455 threads, the last wave 7 lanes wide
    (1, 512, 32, 0, 8), (1, 513, 32, 0, 8),       # 64 and 65 chunks: the fused finalize's limit
    (1, 2100, 32, 0, 8),                  # 263 chunks: the strided loop of the finalize kernel
    (4, 5000, 32, 0, 8),                  # 26 rows per chunk, 193 chunks, the last with 8 rows
    GN_HUGE,                              # the 1024-row cap: 1025 chunks, the last with 37 rows.  Plain only
    (128, 4, 64, 0, 32),                  # many images
]
GN_FUSE_MAX_CHUNKS = 64
GN_CHUNKS = {(1, 512): 64, (1, 513): 65, (1, 2100): 263, (4, 5000): 193, (1, 2 ** 20 + 37): 1025, (2, 100): 13}
GN_GATHER_SPLIT = 60                      # rows of GN_LADDER kept locally in the gathered form (the other 40 arrive as partials)


def gn_chunks(rows, nimg):
    """norm.hip's gn_stat_rows restated (tests/test_norm_kernels_gpu.py holds it against vsx_groupnorm_chunks)"""
    rpc = min(max(rows * nimg // 768, 8), 1024)
    return (rows + rpc - 1) // rpc


def gn_runs(with_huge=True):
    """(nimg, rows, C1, C2, groups, rung, silu, eps, zero group)"""
    runs = []
    for c in GN_CASES:
        if c == GN_HUGE:
            if with_huge:
                runs.append(c + (0, False, 1e-5, False))
            continue
        runs += [c + (0, False, 1e-5, False), c + (0, True, 1e-5, False), c + (0, True, 1e-6, False)]
    runs += [GN_ZERO + (0, False, 1e-5, True), GN_ZERO + (0, True, 1e-5, True)]
    runs += [GN_LADDER + (r, False, 1e-5, False) for r in RUNGS if r]
    runs += [GN_ZERO + ('tiny', False, 1e-5, False), GN_ZERO + ('tiny', True, 1e-6, False)]
    return runs


def gn_id(run):
    return ('-'.join(str(v) for v in run[:5]) + _rtag(run[5]) + ('-silu' if run[6] else '')
            + ('' if run[7] == 1e-5 else '-eps1e-6') + ('-zerogroup' if run[8] else ''))


def gn_inputs(run, device):
    nimg, rows, C1, C2, groups, rung, _, _, zero = run
    g = _gen(nimg, rows, C1, C2, groups, 99 if rung == 'tiny' else rung)
    x = rung_tensor(g, rung, nimg, rows, C1)
    x2 = rung_tensor(g, rung, nimg, rows, C2) if C2 else None
    if zero:
        cpg = C1 // groups
        x[1, :, 5 * cpg:6 * cpg] = 0.0
    gamma, beta = _randn(g, C1 + C2, scale=0.2, shift=1.0), _randn(g, C1 + C2, scale=0.1)
    mv = (lambda t: None if t is None else t.to(device))
    return mv(x), mv(x2), mv(gamma), mv(beta)


def run_group_norm(impl, device, run, fn=None, rule='form'):
    """`fn` replaces impl.group_norm (the mutants); rule 'two_pass': the plain rule, no form ideal"""
    nimg, rows, C1, C2, groups, rung, silu, eps, zero = run
    x, x2, gamma, beta = gn_inputs(run, device)
    fn = fn or impl.group_norm
    got = fn(x, gamma, beta, groups, eps, nimg, silu=silu, x2=x2)
    assert got.shape == (nimg, rows, C1 + C2) and got.dtype == H
    if impl is not None and gn_chunks(rows, nimg) <= GN_FUSE_MAX_CHUNKS:
        try:
            impl.set_option('gn_fuse', 1)
            fused = fn(x, gamma, beta, groups, eps, nimg, silu=silu, x2=x2)
        finally:
            impl.set_option('gn_fuse', 0)
        assert torch.equal(got, fused), 'statistics finalized inside the apply kernel: other bits'
    if zero:
        cpg = C1 // groups
        bz = beta[5 * cpg:6 * cpg]
        if silu:                      # plain PyTorch, not the project's own silu kernel: fp32 beta * sigmoid(beta), rounded to fp16
            bz = (bz.float() * torch.sigmoid(bz.float())).to(H)
        assert torch.equal(got[1, :, 5 * cpg:6 * cpg], bz.expand(rows, cpg)), 'a group of zeros must come out as beta, bit for bit'
    want = ref_group_norm(x, x2, gamma, beta, groups, eps, nimg, silu, torch.float64)
    ideal = ref_group_norm(x, x2, gamma, beta, groups, eps, nimg, silu, torch.float32).to(H)
    name = 'group_norm ' + gn_id(run)
    if rule == 'two_pass':
        return check(name, got, want, ideal, 'group_norm', _rid(rung))
    form = form_group_norm(x, x2, gamma, beta, groups, eps, nimg, silu)
    return check_form(name, got, want, ideal, form, SPREAD['group_norm'], 'group_norm', _rid(rung))


def host_partials(xb, nimg, groups):
    """what vsx_groupnorm_stats hands over, as one chunk: [nimg, 1, groups, 2] fp32"""
    xs = xb.float().reshape(nimg, -1, groups, xb.shape[-1] // groups)
    return torch.stack([xs.sum((1, 3)), (xs * xs).sum((1, 3))], dim=-1)[:, None].contiguous()


GATHER_RUNGS = (0, 3)


def run_group_norm_gathered(impl, device, rung, partials, fn=None):
    """the frame-sharded form: the rows of GN_LADDER split in two; the second part arrives as partial sums
    (`partials(xb, nimg, groups)`) through `partial_hook`, count_rows = all rows; against the reference over ALL rows"""
    nimg, rows, C1, _, groups = GN_LADDER
    x, _, gamma, beta = gn_inputs(GN_LADDER + (rung, False, EPS, False), device)
    xa, xb = x[:, :GN_GATHER_SPLIT].contiguous(), x[:, GN_GATHER_SPLIT:].contiguous()
    other = partials(xb, nimg, groups)
    seen = []

    def hook(p):
        seen.append(p.shape[1])
        return torch.cat([p, other], dim=1).contiguous()
    got = (fn or impl.group_norm)(xa, gamma, beta, groups, EPS, nimg, partial_hook=hook, count_rows=rows)
    assert seen and got.shape == xa.shape
    want = ref_group_norm(x, None, gamma, beta, groups, EPS, nimg, False, torch.float64)[:, :GN_GATHER_SPLIT].contiguous()
    ideal = ref_group_norm(x, None, gamma, beta, groups, EPS, nimg, False, torch.float32).to(H)[:, :GN_GATHER_SPLIT].contiguous()
    form = form_group_norm(x, None, gamma, beta, groups, EPS, nimg, False)[:, :GN_GATHER_SPLIT].contiguous()
    return check_form(f'group_norm gathered {GN_GATHER_SPLIT}+{rows - GN_GATHER_SPLIT} rows {rung_of(rung)[0]}', got, want, ideal,
                      form, SPREAD['group_norm'], 'group_norm_gathered', _rid(rung))


# ------------------------------------------------------------------------------------------------
# LayerNorm forward and the row statistics.  (M, C, rows_per_frame, frames, frame_offset, rung)
# ------------------------------------------------------------------------------------------------
LN_SHAPES = [(1, 8), (3, 64), (5, 72), (17, 320), (16, 504), (9, 512), (9, 520), (7, 640), (5, 1024), (5, 1032), (33, 1280),
             (3, 2048), (1001, 320)]            # 512 | 520 and 1024 | 1032: the dispatch boundaries; 17, 9, 5, 3, 1001: ragged
LN_PE = [(48, 320, 6, 4, 2), (24, 64, 1, 24, 0), (10, 1280, 5, 1, 3)]      # against the 16 / 8 / 4 rows of a workgroup
LN_LADDER = (17, 320)
LN_RUNS = ([s + (0, 0, 0, 0) for s in LN_SHAPES] + [p + (0,) for p in LN_PE] + [LN_LADDER + (0, 0, 0, r) for r in RUNGS if r]
           + [LN_LADDER + (0, 0, 0, 'tiny')])
RS_RUNS = [s + (0,) for s in LN_SHAPES] + [LN_LADDER + (r,) for r in RUNGS if r] + [LN_LADDER + ('tiny',)]


def ln_id(run):
    M, C, rpf, frames, off, rung = run
    return f'{M}x{C}' + (f'-pe{rpf}x{frames}+{off}' if rpf else '') + _rtag(rung)


def rs_id(run):
    return f'{run[0]}x{run[1]}' + _rtag(run[2])


def ln_inputs(M, C, rung, device, table=0):
    g = _gen(M, C, 99 if rung == 'tiny' else rung, table)
    x = rung_tensor(g, rung, M, C)
    gamma, beta = _randn(g, C, scale=0.2, shift=1.0), _randn(g, C, scale=0.1)
    pe = _randn(g, table, C, scale=0.5).to(device) if table else None
    return x.to(device), gamma.to(device), beta.to(device), pe


def run_layer_norm(impl, device, run, fn=None):
    M, C, rpf, frames, off, rung = run
    x, gamma, beta, pe = ln_inputs(M, C, rung, device, table=off + frames + 1 if rpf else 0)
    got = (fn or impl.layer_norm)(x, gamma, beta, EPS, pe=pe, rows_per_frame=rpf, frames=frames, frame_offset=off)
    assert got.shape == x.shape and got.dtype == H
    want = ref_layer_norm(x, gamma, beta, EPS, torch.float64, pe, rpf, frames, off)
    ideal = ref_layer_norm(x, gamma, beta, EPS, torch.float32, pe, rpf, frames, off).to(H)
    return check('layer_norm ' + ln_id(run), got, want, ideal, 'layer_norm', _rid(rung))


def run_row_stats(fn, device, run):
    """fn(x, eps) -> [M, 2] fp32"""
    M, C, rung = run
    x = ln_inputs(M, C, rung, device)[0]
    got = fn(x, EPS)
    return check_stats('row_stats ' + rs_id(run), got, ref_row_stats(x, EPS, torch.float64), ref_row_stats(x, EPS, torch.float32),
                       kernel='row_stats', rung=_rid(rung))


# vsx_row_stats_combine: (M, C, split, rung).  Splits: the column parts the GEMM epilogues really write
def split_edges(C, split):
    if split == 'gemm':                   # the persistent kernel: 64, 64, 32 per 160 columns
        return [h * 160 + o for h in range(C // 160) for o in (0, 64, 128)] + [C]
    if split == 'ws':                     # the weight-stationary K = N = 320 kernel: a part per wave = 32 columns
        return list(range(0, C + 1, 32))
    n = int(split)                        # n equal parts
    return [C * i // n for i in range(n + 1)]


COMBINE_SHAPES = [(17, 320), (1001, 320), (7, 640), (33, 1280)]
COMBINE_LADDER = (1001, 320)
COMBINE_RUNS = ([s + ('gemm', 0) for s in COMBINE_SHAPES] + [(17, 320, 'ws', 0), (1001, 320, 'ws', 0)]
                + [s + (n, 0) for s in ((17, 320), (33, 1280)) for n in ('1', '64')]
                + [COMBINE_LADDER + ('gemm', r) for r in RUNGS if r] + [(17, 320, 'gemm', 'tiny')])


def combine_id(run):
    return f'{run[0]}x{run[1]}-{run[2]}' + _rtag(run[3])


def combine_parts(x, split):
    """[M, nparts, 2] fp32 (sum, sum of squares) of the column parts, in fp32 PyTorch"""
    xf = x.float()
    e = split_edges(x.shape[-1], split)
    return torch.stack([torch.stack([xf[:, a:b].sum(1), (xf[:, a:b] ** 2).sum(1)], dim=-1) for a, b in zip(e[:-1], e[1:])],
                       dim=1).contiguous()


def run_row_stats_combine(fn, device, run):
    """fn(parts [M, nparts, 2], C, eps) -> [M, 2] fp32"""
    M, C, split, rung = run
    x = ln_inputs(M, C, rung, device)[0]
    parts = combine_parts(x, split)
    got = fn(parts, C, EPS)
    return check_stats('row_stats_combine ' + combine_id(run), got, ref_row_stats(x, EPS, torch.float64),
                       ref_row_stats(x, EPS, torch.float32), form_row_stats(x, EPS), SPREAD['row_stats_combine'],
                       kernel='row_stats_combine', rung=_rid(rung))


# ------------------------------------------------------------------------------------------------
# LayerNorm folded into the consuming Linear (ops.DeferredLN): tile-kernel sized.  (M, K, N, kind)
# ------------------------------------------------------------------------------------------------
FOLD_CASES = [(77, 768, 320, 'plain'), (100, 320, 960, 'pe'), (64, 320, 640, 'geglu')]
FOLD_RUNS = [c + (r,) for c in FOLD_CASES for r in RUNGS] + [(77, 768, 320, 'residual', 0)]
FOLD_PE = (5, 4, 2)                        # rows per frame, frames, frame offset
# Where the fold is held to the FORM rule instead of the unchanged two-pass rule: kind -> rungs.  Only where the float32 restatement
# of the fold's algebraic form (form_ln_linear: W' = fp16(W o gamma), c2 = fp16(beta W^T + b), the fp16 rows pe W^T) ITSELF misses
# the two-pass rule, which tests/test_norm_case.py holds this table against on the references alone:
#   plain, residual  never: the restatement is at 1.41 x the ideal's rel-L2 and 0.9 of the per-element bound on every rung
#   pe               uniform*0.5+16 and randn+64: its worst element is at 1.03 of the per-element bound (the third fp16 operand)
#   geglu            every rung, the base included: the operand roundings pass through h * gelu(g); rel-L2 1.73 x, element 1.6 - 3.1 x
# Everywhere else the fold must meet what a materialised fp32 LayerNorm -> Linear meets.  Both sets of figures are recorded always.
FOLD_FORM_RUNGS = {'plain': (), 'residual': (), 'pe': (4, 6), 'geglu': tuple(RUNGS)}


def fold_id(run):
    return f'{run[0]}x{run[1]}x{run[2]}-{run[3]}' + _rtag(run[4])


def run_folded(fn, device, run):
    """fn(x, gamma, beta, eps, pe, rows_per_frame, frames, frame_offset, w, b, residual, geglu) -> [M, N] fp16"""
    M, K, N, kind, rung = run
    rpf, frames, off = FOLD_PE if kind == 'pe' else (0, 0, 0)
    x, gamma, beta, pe = ln_inputs(M, K, rung, device, table=off + frames + 1 if rpf else 0)
    g = _gen(M, K, N, rung, 7)
    nw = 2 * N if kind == 'geglu' else N
    w, b = _randn(g, nw, K, scale=K ** -0.5).to(device), _randn(g, nw, scale=0.5).to(device)
    res = _randn(g, M, N).to(device) if kind == 'residual' else None
    got = fn(x, gamma, beta, EPS, pe, rpf, frames, off, w, b, res, kind == 'geglu')
    assert got.shape == (M, N) and got.dtype == H
    kw = dict(pe=pe, rows_per_frame=rpf, frames=frames, frame_offset=off, residual=res, geglu=kind == 'geglu')
    want = ref_ln_linear(x, gamma, beta, EPS, w, b, torch.float64, **kw)
    ideal = ref_ln_linear(x, gamma, beta, EPS, w, b, torch.float32, **kw).to(H)
    form = form_ln_linear(x, gamma, beta, EPS, w, b, **kw)
    return check_form('folded_layer_norm ' + fold_id(run), got, want, ideal, form, SPREAD['folded'], 'folded_layer_norm ' + kind, _rid(rung),
                      use_form=rung in FOLD_FORM_RUNGS[kind])


# ------------------------------------------------------------------------------------------------
# SPREAD, measured on the references alone
# ------------------------------------------------------------------------------------------------
def _ratios(per_order):
    """{order: {metric: value}} -> {metric: largest / smallest over the orders}"""
    out = {}
    for m in next(iter(per_order.values())):
        vals = [v[m] for v in per_order.values()]
        out[m] = max(vals) / max(min(vals), 1e-300)
    return out


def measure_spread(which):
    """-> ({metric: the largest ratio between two summation orders of the form ideal over the ladder}, the per-rung table)"""
    table = {}
    for rung in RUNGS:
        per = {}
        if which == 'group_norm':
            nimg, rows, C1, C2, groups = GN_LADDER
            x, x2, gamma, beta = gn_inputs(GN_LADDER + (rung, False, EPS, False), 'cpu')
            want = ref_group_norm(x, x2, gamma, beta, groups, EPS, nimg, False, torch.float64)
            ideal = ref_group_norm(x, x2, gamma, beta, groups, EPS, nimg, False, torch.float32).to(H)
            for o in ORDERS:
                f = measure(form_group_norm(x, x2, gamma, beta, groups, EPS, nimg, False, order=o), want, ideal)[0]
                per[o] = {m: f[m + '_kernel'] for m in METRICS}
        elif which == 'row_stats_combine':
            x = ln_inputs(*COMBINE_LADDER, rung, 'cpu')[0]
            want = ref_row_stats(x, EPS, torch.float64)
            for o in ORDERS:
                e = _stat_err(form_row_stats(x, EPS, order=o), want)
                per[o] = {'rstd': e[0], 'shift': e[1]}
        else:
            M, K, N, kind = FOLD_CASES[0]
            x, gamma, beta, _ = ln_inputs(M, K, rung, 'cpu')
            g = _gen(M, K, N, rung, 7)
            w, b = _randn(g, N, K, scale=K ** -0.5), _randn(g, N, scale=0.5)
            want = ref_ln_linear(x, gamma, beta, EPS, w, b, torch.float64)
            ideal = ref_ln_linear(x, gamma, beta, EPS, w, b, torch.float32).to(H)
            for o in ORDERS:
                f = measure(form_ln_linear(x, gamma, beta, EPS, w, b, order=o), want, ideal)[0]
                per[o] = {m: f[m + '_kernel'] for m in METRICS}
        table[LADDER[rung][0]] = _ratios(per)
    return {m: max(t[m] for t in table.values()) for m in next(iter(table.values()))}, table


# ------------------------------------------------------------------------------------------------
# the scalar glue of csrc/elementwise.hip
# ------------------------------------------------------------------------------------------------
EW_SIZES = [1, 255, 256, 257, 33001]
# (alpha_t, alpha_next): both ends of the DDIM schedule (alphas_cumprod of the scaled-linear 1000-step schedule runs from
# 0.99915 down to 0.00466; the last step goes to alpha_next = 1) and a middle step
DDIM_ALPHAS = [(0.00466, 0.00583), (0.37, 0.52), (0.99915, 1.0)]
DDIM_GUIDANCE = [None, 0.0, 1.0, 7.5]             # None: eps_c = None
DDIM_REFUSED = [(0.0, 0.5), (-0.1, 0.5), (1.5, 0.5), (0.5, 0.0), (0.5, 1.0001), (0.5, -1.0)]
AXPY_S = [1.0, 0.5, -0.18215]


def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def ref_cfg_ddim(x, eu, ec, guidance, alpha_t, alpha_next, dt):
    """the scalars as the C ABI receives them (floats), everything else in `dt`"""
    a_t, a_n = torch.tensor(_f32(alpha_t), dtype=dt), torch.tensor(_f32(alpha_next), dtype=dt)
    e = eu.to(dt)
    if ec is not None:
        e = e + torch.tensor(_f32(guidance), dtype=dt) * (ec.to(dt) - e)
    x0 = (x.to(dt) - (1 - a_t).sqrt() * e) / a_t.sqrt()
    return a_n.sqrt() * x0 + (1 - a_n).sqrt() * e


def run_cfg_ddim(impl, device, n, alphas, guidance):
    g = _gen(n, int(alphas[0] * 1e5), -1 if guidance is None else int(guidance * 10))
    x, eu, ec = (_randn(g, n).to(device) for _ in range(3))
    if guidance is None:
        ec = None
    got = impl.cfg_ddim_step(x, eu, ec, 1.0 if guidance is None else guidance, alphas[0], alphas[1])
    want = ref_cfg_ddim(x, eu, ec, guidance, alphas[0], alphas[1], torch.float64)
    ideal = ref_cfg_ddim(x, eu, ec, guidance, alphas[0], alphas[1], torch.float32).to(H)
    return check(f'cfg_ddim_step n={n} alphas={alphas} guidance={guidance}', got, want, ideal)


def run_masked_blend(impl, device, n):
    C = 3
    g = _gen(n, 11)
    x, src = _randn(g, C, n, scale=2.0).to(device), _randn(g, C, n, scale=2.0).to(device)
    hard = (torch.rand(n, generator=g) > 0.5).to(H).to(device)
    out = impl.masked_blend(x, src, hard)
    assert torch.equal(out, torch.where(hard.bool()[None, :], x, src)), 'a 0 / 1 mask must return x or src bit for bit'
    soft = torch.rand(n, generator=g).to(H).to(device)
    got = impl.masked_blend(x, src, soft)
    ref = (lambda dt: src.to(dt) + soft.to(dt)[None, :] * (x.to(dt) - src.to(dt)))
    return check(f'masked_blend n={n}', got, ref(torch.float64), ref(torch.float32).to(H))


def run_axpy(impl, device, n, s):
    g = _gen(n, int(s * 1e5) + 10 ** 6)
    a, b = _randn(g, n, scale=3.0).to(device), _randn(g, n, scale=3.0).to(device)
    got = impl.axpy(a, b, s)
    ref = (lambda dt: a.to(dt) + torch.tensor(_f32(s), dtype=dt) * b.to(dt))
    return check(f'axpy n={n} s={s}', got, ref(torch.float64), ref(torch.float32).to(H))


PACK_CASES = [(2, 4, 3, 6, 10, 8), (1, 8, 1, 16, 17, 8), (2, 3, 3, 1, 1, 8)]       # (B, Cin, F, H, W, Cpad): Cin < Cpad; Cin = Cpad,
UNPACK_CASES = [(2, 3, 6, 10, 8, 4), (1, 2, 16, 17, 4, 4), (2, 3, 1, 1, 8, 3)]     # HW = 272; one pixel.  (B, F, H, W, Cs, Cout)


def run_pack(impl, device, case):
    B, Cin, Fr, Hh, W, cpad = case
    x = _randn(_gen(*case), B, Cin, Fr, Hh, W).to(device)
    got = impl.pack_latents(x, cpad)
    want = torch.zeros(B * Fr, Hh, W, cpad, dtype=H, device=device)
    want[..., :Cin] = x.permute(0, 2, 3, 4, 1).reshape(B * Fr, Hh, W, Cin)
    assert got.shape == want.shape and torch.equal(got, want)


def run_unpack(impl, device, case):
    B, Fr, Hh, W, Cs, cout = case
    x = _randn(_gen(*case, 1), B * Fr, Hh, W, Cs).to(device)
    got = impl.unpack_latents(x, B, cout)
    want = x[..., :cout].reshape(B, Fr, Hh, W, cout).permute(0, 4, 1, 2, 3).contiguous()
    assert got.shape == want.shape and torch.equal(got, want)


def expected_figures(with_huge=True, gathered=True):
    """how many entries a full pass over the tables leaves in FIGURES"""
    return (len(gn_runs(with_huge)) + (len(GATHER_RUNGS) if gathered else 0) + len(LN_RUNS) + len(RS_RUNS) + len(COMBINE_RUNS)
            + len(FOLD_RUNS) + len(EW_SIZES) * (len(DDIM_ALPHAS) * len(DDIM_GUIDANCE) + 1 + len(AXPY_S)))
