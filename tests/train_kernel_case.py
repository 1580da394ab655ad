"""Shared by tests/test_train_kernels_gpu.py (the HIP kernels) and tests/test_train_kernel_case.py (the CPU stand-ins of
tests/host_emulation.py and deliberate mutants of them): the case tables of the training-step kernels
(videoswap_amd/csrc/train.hip, plus quick_gelu / silu and the row softmaxes), fp64 references of every op on
fp16-exact inputs in plain PyTorch, and ONE comparison rule.  No kernels and no GPU calls of its own: every runner takes
`impl` (videoswap_amd.ops or host_emulation) and a device.

The rule fixes no tolerance in advance.  `want` is the reference in float64, `ideal` the same reference in float32 rounded
to fp16 (what a perfect fp32 kernel would store), `got` the result under test:

    tensor rel-L2       err(got) <= 1.5 x err(ideal)
    worst row rel-L2    <= 2 x the ideal's worst row (rows = last axis, >= 8 wide; a row whose reference norm is below
                        10 % of the mean row norm is measured against that floor, as `rel_err` of test_kernels_gpu.py)
    max-abs             <= 4 x the ideal's
    per element         |got - want| <= 1 fp16 ulp(want) + 2^-10 rms(want's row)
    got                 finite everywhere

1.5 x and 2 x cover another summation order and v_rcp / v_exp against IEEE division; the ulp term is the output rounding,
the rms term the fp32 cancellation in gz - m1 - xhat m2 (a thousand times below a wrong element).  For the element-wise
GELU / SiLU kernels the rms term is replaced by 1e-5 |d| max(1, |h|, |g|): ten times the documented 3e-7 of the erf form
(csrc/common.h) plus the error of __expf, scaled by the factors the activation is multiplied with.
"""
import math

import torch
import torch.nn.functional as F

H = torch.float16
EPS = 1e-5
FIGURES = []                    # one dict per compared tensor, appended by `check`


# ------------------------------------------------------------------------------------------------
# the comparison rule
# ------------------------------------------------------------------------------------------------
def ulp16(want):
    """spacing of fp16 at |want| (float64 tensor); 2^-24 in the subnormal range"""
    a = want.double().abs()
    _, e = torch.frexp(a.clamp_min(2.0 ** -14))                 # a = m 2^e with m in [0.5, 1)
    return torch.exp2(e.double() - 11)


def _l2(d, want):
    return float(d.norm() / want.norm().clamp_min(1e-30))


def _worst_row(d, want):
    if want.dim() < 2 or want.shape[-1] < 8:
        return 0.0
    dr, rr = d.reshape(-1, d.shape[-1]).norm(dim=1), want.reshape(-1, want.shape[-1]).norm(dim=1)
    return float((dr / rr.clamp_min(0.1 * rr.mean().clamp_min(1e-12))).max())


def measure(got, want, ideal, elem_extra=None):
    """-> (figures, names of the metrics that fail)"""
    assert got.shape == want.shape == ideal.shape, (tuple(got.shape), tuple(want.shape), tuple(ideal.shape))
    assert got.dtype == H and ideal.dtype == H and want.dtype == torch.float64
    if want.numel() == 0:
        return {'empty': True}, []
    dg, di = got.double() - want, ideal.double() - want
    if elem_extra is None:
        elem_extra = 2.0 ** -10 * want.pow(2).mean(-1, keepdim=True).sqrt()
    elem_bound = ulp16(want) + elem_extra.double()
    fig = {'l2_ideal': _l2(di, want), 'l2_kernel': _l2(dg, want),
           'row_ideal': _worst_row(di, want), 'row_kernel': _worst_row(dg, want),
           'maxabs_ideal': float(di.abs().max()), 'maxabs_kernel': float(dg.abs().max()),
           'elem_ideal': float((di.abs() / elem_bound).max()), 'elem_kernel': float((dg.abs() / elem_bound).max()),
           'finite': bool(torch.isfinite(got).all())}
    fig.update(l2_bound=1.5 * fig['l2_ideal'], row_bound=2 * fig['row_ideal'], maxabs_bound=4 * fig['maxabs_ideal'],
               elem_bound=1.0)
    failed = [m for m in ('l2', 'row', 'maxabs', 'elem') if not fig[m + '_kernel'] <= fig[m + '_bound']]
    if not fig['finite']:
        failed.append('finite')
    return fig, failed


def check(name, got, want, ideal, elem_extra=None):
    fig, failed = measure(got, want, ideal, elem_extra)
    fig = dict(case=name, **fig)
    print(' '.join(f'{k}={v:.3e}' if isinstance(v, float) else f'{k}={v}' for k, v in fig.items()))
    FIGURES.append(fig)
    assert not failed, (name, failed, fig)
    return fig


def _gen(*key):
    return torch.Generator().manual_seed(abs(hash(tuple(int(k) for k in key))) % (2 ** 31))


def _randn(g, *shape, scale=1.0, shift=0.0):
    return (torch.randn(*shape, generator=g) * scale + shift).to(H)


# ------------------------------------------------------------------------------------------------
# references: every one takes fp16 tensors and a dtype (float64: `want`; float32, rounded to fp16: `ideal`)
# ------------------------------------------------------------------------------------------------
def _cdf_pdf(g):
    return 0.5 * torch.erfc(-g * 0.7071067811865476), torch.exp(-0.5 * g * g) * 0.3989422804014327


def ref_geglu_fwd(y2, dt):
    h, g = y2.to(dt).chunk(2, dim=-1)
    return h * g * _cdf_pdf(g)[0]


def ref_geglu_bwd(dout, y2, dt):
    h, g = y2.to(dt).chunk(2, dim=-1)
    cdf, pdf = _cdf_pdf(g)
    d = dout.to(dt)
    return torch.cat([d * g * cdf, d * h * (cdf + g * pdf)], dim=-1)


def ref_silu(x, dt):
    x = x.to(dt)
    return x * torch.sigmoid(x)


def ref_quick_gelu(x, dt):
    x = x.to(dt)
    return x * torch.sigmoid(1.702 * x)


def ref_silu_bwd(dy, x, dt):
    x = x.to(dt)
    s = torch.sigmoid(x)
    return dy.to(dt) * (s + x * s * (1.0 - s))


def ref_group_norm_bwd(dy, x, x2, gamma, beta, groups, eps, nimg, silu, dt):
    """autograd through a two-pass GroupNorm(+SiLU) in `dt` -> d(x | x2) [nimg, rows, C1 + C2]"""
    xin = (x if x2 is None else torch.cat([x, x2], dim=-1)).to(dt).requires_grad_(True)
    C = xin.shape[-1]
    with torch.enable_grad():
        xs = xin.reshape(nimg, -1, groups, C // groups)
        mean = xs.mean((1, 3), keepdim=True)
        var = xs.var((1, 3), unbiased=False, keepdim=True)
        y = ((xs - mean) * (var + eps).rsqrt()).reshape(nimg, -1, C) * gamma.to(dt) + beta.to(dt)
        if silu:
            y = F.silu(y)
        (g,) = torch.autograd.grad(y, xin, dy.to(dt).reshape(y.shape))
    return g.reshape(xin.shape)


def ref_layer_norm_bwd(dy, x, gamma, eps, dt):
    xf = x.to(dt).requires_grad_(True)
    with torch.enable_grad():
        y = F.layer_norm(xf, (x.shape[-1],), gamma.to(dt), None, eps)
        (g,) = torch.autograd.grad(y, xf, dy.to(dt))
    return g


def ref_softmax_bwd(p, dp, scale, dt):
    p, dp = p.to(dt), dp.to(dt)
    return scale * p * (dp - (dp * p).sum(-1, keepdim=True))


def ref_sum_pool2x2(x, dt):
    n, h2, w2, c = x.shape
    return x.to(dt).view(n, h2 // 2, 2, w2 // 2, 2, c).sum((2, 4))


def ref_softmax_rows(s, rows_per_seq, dt):
    s = s.to(dt)
    if rows_per_seq is not None:
        nk = s.shape[-1]
        q = (torch.arange(s.numel() // nk, device=s.device) % rows_per_seq).view(*s.shape[:-1], 1)
        s = s.masked_fill(torch.arange(nk, device=s.device) > q, float('-inf'))
    return s.softmax(-1)


def _r16(v):
    return torch.tensor(v, dtype=torch.float32).to(H).float().item()


def ref_adapter_gather(tracks, selected, dmap, rate, out_scale, dt):
    """the fp16-rounded sub-pixel positions and weights of vsx_adapter_scatter, restated as tests/host_emulation.py does;
    the accumulation in `dt`"""
    Fr, P = tracks.shape[:2]
    _, h, w, C = dmap.shape
    out = torch.zeros(P, C, dtype=dt, device=dmap.device)
    tr, sel = tracks.cpu(), selected.cpu()
    for f in range(Fr):
        for pt in range(P):
            if not int(sel[pt]):
                continue
            px, py = float(tr[f, pt, 0]), float(tr[f, pt, 1])
            if px < 0 or py < 0:
                continue
            x, y = _r16(_r16(px) / rate), _r16(_r16(py) / rate)
            x1, y1 = int(x), int(y)
            x2, y2 = x1 + 1, y1 + 1
            xf, yf = _r16(x - x1), _r16(y - y1)
            x1, x2 = max(min(x1, w - 1), 0), max(min(x2, w - 1), 0)
            y1, y2 = max(min(y1, h - 1), 0), max(min(y2, h - 1), 0)
            xm, ym = _r16(1.0 - xf), _r16(1.0 - yf)
            wgt = [_r16(xm * ym), _r16(xf * ym), _r16(xm * yf), _r16(xf * yf)]
            for (xx, yy), wg in zip(((x1, y1), (x2, y1), (x1, y2), (x2, y2)), wgt):
                out[pt] += wg * dmap[f, yy, xx].to(dt)
    return out * out_scale


# ------------------------------------------------------------------------------------------------
# GroupNorm backward.  (nimg, rows, C1, C2, groups, variant): the path each case reaches is named beside it
# ------------------------------------------------------------------------------------------------
GN_CASES = [
    (3, 50, 64, 0, 32, 'both'),           # ragged last chunk: 64 row slots hold at most 8 rows
    (2, 100, 320, 0, 32, 'both'),         # idle threads (480 of 512 active), cpg = 10: 16-byte vectors straddle groups
    (2, 77, 640, 320, 32, 'both'),        # concat, cpg = 30
    (2, 40, 1280, 1280, 32, 'both'),      # rp = 1
    (1, 17, 4096, 0, 32, 'both'),         # both 4096-float LDS arrays full
    (1, 16, 2048, 0, 256, 'both'),        # the maximum number of groups
    (2, 33, 32, 0, 1, 'both'),            # one group
    (128, 4, 64, 0, 32, 'both'),          # many images
    (1, 2100, 32, 0, 8, 'both'),          # 263 chunks: the strided loop of the finalize kernel
    (4, 5000, 32, 0, 8, 'both'),          # 9 rows per chunk, 556 chunks, the last with 5 rows
    (1, 2 ** 20 + 37, 8, 0, 2, 'plain'),  # 512 rows per chunk (the cap)
    (2, 100, 320, 0, 32, 'shifted'),      # x = uniform * 0.5 + 8: the one-pass variance
]
GN_HUGE = GN_CASES[10]


def gn_runs(cases=GN_CASES):
    return [c[:5] + (v, s) for c in cases for v, s in
            {'both': (('randn', False), ('randn', True)), 'plain': (('randn', False),),
             'shifted': (('shifted', False), ('shifted', True))}[c[5]]]


def gn_id(run):
    return '-'.join(str(v) for v in run[:5]) + ('-shifted' if run[5] == 'shifted' else '') + ('-silu' if run[6] else '')


def gn_inputs(run, device):
    nimg, rows, C1, C2, groups, kind, _ = run
    g = _gen(nimg, rows, C1, C2, groups, kind == 'shifted')
    if kind == 'shifted':
        x = (torch.rand(nimg, rows, C1, generator=g) * 0.5 + 8.0).to(H)
    else:
        x = _randn(g, nimg, rows, C1, scale=1.5, shift=0.3)
    x2 = _randn(g, nimg, rows, C2, scale=1.5, shift=0.3) if C2 else None
    dy = _randn(g, nimg, rows, C1 + C2)
    gamma, beta = _randn(g, C1 + C2, scale=0.2, shift=1.0), _randn(g, C1 + C2, scale=0.1)
    mv = (lambda t: None if t is None else t.to(device))
    return mv(dy), mv(x), mv(x2), mv(gamma), mv(beta)


def run_group_norm_bwd(impl, device, run, fn=None):
    """`fn`: replaces impl.group_norm_bwd (the mutants of tests/test_train_kernel_case.py)"""
    nimg, rows, C1, C2, groups, _, silu = run
    dy, x, x2, gamma, beta = gn_inputs(run, device)
    fn = fn or impl.group_norm_bwd
    dx, dx2 = fn(dy, x, gamma, beta, groups, EPS, nimg, silu=silu, x2=x2)
    ax, ax2 = fn(dy, x, gamma, beta, groups, EPS, nimg, silu=silu, x2=x2)
    assert torch.equal(dx, ax) and (dx2 is None or torch.equal(dx2, ax2)), 'a second call differs: not deterministic'
    want = ref_group_norm_bwd(dy, x, x2, gamma, beta, groups, EPS, nimg, silu, torch.float64)
    ideal = ref_group_norm_bwd(dy, x, x2, gamma, beta, groups, EPS, nimg, silu, torch.float32).to(H)
    name = 'group_norm_bwd ' + gn_id(run)
    figs = [check(name + ' dx', dx, want[..., :C1].contiguous(), ideal[..., :C1].contiguous())]
    if C2:
        figs.append(check(name + ' dx2', dx2, want[..., C1:].contiguous(), ideal[..., C1:].contiguous()))
    else:
        assert dx2 is None
    return figs


# ------------------------------------------------------------------------------------------------
# LayerNorm backward: (M, C, mean of the rows)
# ------------------------------------------------------------------------------------------------
LN_CASES = [(1, 8, 0.5), (3, 64, 0.5), (5, 72, 0.5), (1001, 320, 0.5), (7, 640, 0.5), (33, 1280, 0.5), (4, 2048, 0.5),
            (6, 320, 8.0),                        # rows with mean 8
            (5, 7, 0.5), (2, 2500, 0.5)]          # any C > 0: odd, and beyond 2048


def run_layer_norm_bwd(impl, device, case, fn=None):
    M, C, mean = case
    g = _gen(M, C, int(mean * 10))
    x, dy, gamma = _randn(g, M, C, scale=2.0 if mean < 1 else 0.5, shift=mean), _randn(g, M, C), _randn(g, C, scale=0.2, shift=1.0)
    x, dy, gamma = x.to(device), dy.to(device), gamma.to(device)
    got = (fn or impl.layer_norm_bwd)(dy, x, gamma, EPS)
    want = ref_layer_norm_bwd(dy, x, gamma, EPS, torch.float64)
    ideal = ref_layer_norm_bwd(dy, x, gamma, EPS, torch.float32).to(H)
    return check(f'layer_norm_bwd {M}x{C} mean {mean:g}', got, want, ideal)


# ------------------------------------------------------------------------------------------------
# softmax backward on row-padded buffers: (nb, heads, nq, nk) x scale
# ------------------------------------------------------------------------------------------------
SMB_SHAPES = [(1, 1, 1, 1), (1, 2, 5, 13), (2, 1, 3, 64), (1, 1, 7, 65), (2, 8, 9, 77), (1, 2, 6, 203), (1, 1, 3, 1000)]
SMB_CASES = [s + (sc,) for s in SMB_SHAPES for sc in (1.0, 40 ** -0.5)]
SENTINEL = 1234.0


def smb_inputs(case, device):
    nb, heads, nq, nk, _ = case
    g = _gen(nb, heads, nq, nk)
    ld = (nk + 7) // 8 * 8
    nrows = nb * heads * nq
    # rows in turn: peaked (one column 8 above the others: p ~ 0.9 to 0.99), near-uniform, ordinary.  Peaked, not SATURATED:
    # where p = 1 in fp16 every dS of the row is a difference of fp32 roundings near 1e-7, below the ulp term, and the
    # fp32 ideal itself misses the per-element bound (measured: 1.9 x at 65 columns with logits = 8 randn)
    kind = torch.arange(nrows) % 3
    logits = torch.randn(nrows, nk, generator=g) * torch.tensor([1.0, 0.01, 1.0])[kind].view(nrows, 1)
    logits[torch.arange(nrows), torch.arange(nrows) % nk] += 8.0 * (kind == 0)
    pbuf = torch.zeros(nb, heads, nq, ld, dtype=H)
    pbuf[..., :nk] = logits.view(nb, heads, nq, nk).softmax(-1).to(H)
    dbuf = torch.full((nb, heads, nq, ld), SENTINEL, dtype=H)
    dbuf[..., :nk] = _randn(g, nb, heads, nq, nk)
    return pbuf.to(device), dbuf.to(device)


def run_softmax_bwd(impl, device, case, fn=None):
    nb, heads, nq, nk, scale = case
    pbuf, dbuf = smb_inputs(case, device)
    p0, d0 = pbuf.clone(), dbuf.clone()
    out = (fn or impl.softmax_bwd)(pbuf[..., :nk], dbuf[..., :nk], scale)
    assert out.data_ptr() == dbuf.data_ptr() and out.shape == (nb, heads, nq, nk)          # written over dP
    assert torch.equal(pbuf, p0), 'probs changed'
    assert torch.equal(dbuf[..., nk:], d0[..., nk:]), 'the padding columns of dprobs changed'
    want = ref_softmax_bwd(p0[..., :nk], d0[..., :nk], scale, torch.float64)
    ideal = ref_softmax_bwd(p0[..., :nk], d0[..., :nk], scale, torch.float32).to(H)
    return check(f'softmax_bwd {nb}x{heads}x{nq}x{nk} scale {scale:.3f}', dbuf[..., :nk].contiguous(), want, ideal)


# ------------------------------------------------------------------------------------------------
# GEGLU, SiLU, quick-GELU
# ------------------------------------------------------------------------------------------------
GEGLU_CASES = [(1, 8), (37, 24), (257, 1280)]
G_EXTREME = [30.0, -30.0, 0.0, -0.0, 25.0, -21.5, 6.0, -6.0]        # beyond |g| ~ 21 p^16 overflows and rcp returns 0
H_EXTREME = [100.0, -100.0, 100.0, -100.0]
ACT_SIZES = [1, 255, 256, 257, 33001]
X_EXTREME = [65504.0, -65504.0, 100.0, -100.0, 20.0, -20.0, 0.0, -0.0]


def _mix(t, values, step):
    """write `values` (cyclically) at every `step`-th element of the flattened tensor, first element included"""
    flat = t.view(-1)
    idx = torch.arange(0, flat.numel(), step)
    flat[idx] = torch.tensor(values, dtype=H)[torch.arange(idx.numel()) % len(values)]
    return t


def geglu_inputs(case, device):
    M, N = case
    g = _gen(M, N)
    y2, dout = _randn(g, M, 2 * N, scale=2.0), _randn(g, M, N)
    hh, gg = y2[:, :N].clone(), y2[:, N:].clone()
    _mix(gg, G_EXTREME, 1 if M * N <= 8 else 5)
    _mix(hh, H_EXTREME, 1 if M * N <= 8 else 3)
    y2 = torch.cat([hh, gg], dim=-1).contiguous()
    return y2.to(device), dout.to(device)


def run_geglu(impl, device, case):
    M, N = case
    y2, dout = geglu_inputs(case, device)
    h, g, d = y2[:, :N].double().abs(), y2[:, N:].double().abs(), dout.double().abs()
    one = torch.ones_like(g)
    figs = [check(f'geglu_fwd {M}x{N}', impl.geglu_fwd(y2), ref_geglu_fwd(y2, torch.float64),
                  ref_geglu_fwd(y2, torch.float32).to(H), elem_extra=1e-5 * h * torch.maximum(one, g))]
    extra = 1e-5 * d * torch.maximum(one, torch.maximum(h, g))
    figs.append(check(f'geglu_bwd {M}x{N}', impl.geglu_bwd(dout, y2), ref_geglu_bwd(dout, y2, torch.float64),
                      ref_geglu_bwd(dout, y2, torch.float32).to(H), elem_extra=torch.cat([extra, extra], dim=-1)))
    return figs


def act_inputs(n, device):
    g = _gen(n)
    x = _randn(g, n, scale=3.0)
    k = min(n, len(X_EXTREME))
    x[:k] = torch.tensor(X_EXTREME[:k], dtype=H)
    return x.to(device), _randn(g, n).to(device)


def run_activations(impl, device, n):
    x, dy = act_inputs(n, device)
    ax = torch.maximum(torch.ones_like(x, dtype=torch.float64), x.double().abs())
    figs = []
    for name, got, ref, extra in (('silu', impl.silu(x), ref_silu(x, torch.float64), 1e-5 * ax),
                                  ('quick_gelu', impl.quick_gelu(x), ref_quick_gelu(x, torch.float64), 1e-5 * ax),
                                  ('silu_bwd', impl.silu_bwd(dy, x), ref_silu_bwd(dy, x, torch.float64), 1e-5 * dy.double().abs() * ax)):
        assert not bool(torch.isnan(got).any()) and bool(torch.isfinite(got).all()), name
        fn = {'silu': ref_silu, 'quick_gelu': ref_quick_gelu}.get(name)
        ideal = (fn(x, torch.float32) if fn else ref_silu_bwd(dy, x, torch.float32)).to(H)
        figs.append(check(f'{name} n={n}', got, ref, ideal, elem_extra=extra))
    return figs


# ------------------------------------------------------------------------------------------------
# 2x2 sum pool, adapter gather
# ------------------------------------------------------------------------------------------------
POOL_CASES = [(1, 1, 1, 8), (3, 3, 5, 16), (2, 4, 7, 320)]           # (n, h, w, c) of the OUTPUT


def run_sum_pool(impl, device, case):
    n, h, w, c = case
    x = _randn(_gen(n, h, w, c), n, 2 * h, 2 * w, c).to(device)
    got = impl.sum_pool2x2(x)
    want = ref_sum_pool2x2(x, torch.float64)
    assert got.shape == (n, h, w, c)
    assert bool(((got.double() - want).abs() <= ulp16(want)).all()), 'more than 1 fp16 ulp from the fp64 sum'
    return check(f'sum_pool2x2 {n}x{h}x{w}x{c}', got, want, ref_sum_pool2x2(x, torch.float32).to(H))


GATHER_C = [8, 40, 320, 1280]         # the `c += blockDim.x` loop takes 1, 1, 2 and 5 trips
GATHER_GEOM = dict(F=3, h=6, w=7, rate=8.0, out_scale=0.5)
P_GRID, P_EDGE, P_HIDDEN, P_UNSELECTED = 1, 2, 3, 4


def gather_inputs(C, device, P=6):
    F_, h, w, rate = GATHER_GEOM['F'], GATHER_GEOM['h'], GATHER_GEOM['w'], GATHER_GEOM['rate']
    g = _gen(C, P)
    tracks = torch.rand(F_, P, 2, generator=g) * torch.tensor([(w - 1) * rate, (h - 1) * rate])
    selected = torch.ones(P, dtype=torch.int32)
    if P:
        tracks[:, P_GRID] = torch.tensor([2 * rate, 3 * rate])                    # exactly on the grid
        tracks[:, P_EDGE] = torch.tensor([w * rate - 0.125, h * rate - 0.125])     # x2 / y2 clamp at the right / bottom edge
        tracks[:, P_HIDDEN] = -1.0                                                # invisible in every frame
        selected[P_UNSELECTED] = 0
        tracks[1, 5, 0] = -1.0                                                    # one hidden frame of a visible point
    dmap = _randn(g, F_, h, w, C)
    return tracks.to(device), selected.to(device), dmap.to(device)


def run_adapter_gather(impl, device, C):
    tracks, selected, dmap = gather_inputs(C, device)
    rate, scale = GATHER_GEOM['rate'], GATHER_GEOM['out_scale']
    got = impl.adapter_gather(tracks, selected, dmap, rate, out_scale=scale)
    assert got.shape == (6, C) and got.dtype == H
    assert float(got[P_HIDDEN].abs().max()) == 0.0 and float(got[P_UNSELECTED].abs().max()) == 0.0
    want = ref_adapter_gather(tracks, selected, dmap, rate, scale, torch.float64)
    assert float(want[P_GRID].abs().max()) > 0 and float(want[P_EDGE].abs().max()) > 0
    return check(f'adapter_gather C={C}', got, want, ref_adapter_gather(tracks, selected, dmap, rate, scale, torch.float32).to(H))


def run_adapter_gather_empty(impl, device):
    tracks, selected, dmap = gather_inputs(8, device, P=0)
    got = impl.adapter_gather(tracks, selected, dmap, GATHER_GEOM['rate'], out_scale=1.0)
    assert got.shape == (0, 8) and got.dtype == H


def run_adapter_adjoint(impl, device, C=40):
    """<adapter_scatter(feat), dmap> = <feat, adapter_gather(dmap)>: ties the gradient kernel to the forward kernel with no
    restated weights.  Bound: the same gap for the fp32 ideal of both (host_emulation's scatter, the reference gather), x 4."""
    import host_emulation
    tracks, selected, dmap = gather_inputs(C, device)
    feat = _randn(_gen(C, 99), 6, C).to(device)
    h, w, rate, scale = GATHER_GEOM['h'], GATHER_GEOM['w'], GATHER_GEOM['rate'], GATHER_GEOM['out_scale']

    def gap(scat, gath):
        lhs, rhs = float((scat.double() * dmap.double()).sum()), float((feat.double() * gath.double()).sum())
        return abs(lhs - rhs), abs(lhs)
    got, size = gap(impl.adapter_scatter(tracks, selected, feat, h, w, rate, out_scale=scale),
                    impl.adapter_gather(tracks, selected, dmap, rate, out_scale=scale))
    with torch.no_grad():
        ideal_scat = host_emulation.adapter_scatter(tracks.cpu(), selected.cpu(), feat.cpu(), h, w, rate, out_scale=scale)
    ideal, _ = gap(ideal_scat.to(device), ref_adapter_gather(tracks, selected, dmap, rate, scale, torch.float32).to(H))
    fig = {'case': f'adapter adjoint C={C}', 'gap_ideal': ideal, 'gap_kernel': got, 'gap_bound': 4 * ideal, 'inner_product': size}
    print(fig)
    FIGURES.append(fig)
    assert got <= 4 * ideal, fig
    return fig


# ------------------------------------------------------------------------------------------------
# row softmax, plain and causal
# ------------------------------------------------------------------------------------------------
SMR_COLS = [1, 8, 63, 64, 65, 77, 300]
SMR_SEQ, SMR_NSEQ = 77, 3                    # 231 rows: not a multiple of the 4 rows of a workgroup


def run_softmax_rows(impl, device, ncols, causal):
    nrows = SMR_SEQ * SMR_NSEQ
    ld = (ncols + 7) // 8 * 8
    g = _gen(ncols, causal)
    s = _randn(g, nrows, ncols, scale=3.0)
    s[0] = (torch.randn(ncols, generator=g) * 30000).clamp(-60000, 60000).to(H)     # fp16 values up to +-60000
    s[0, ::3] = 60000.0
    s[1] = 3.5                                                                      # all entries equal
    buf = torch.full((SMR_NSEQ, SMR_SEQ, ld), SENTINEL, dtype=H)
    buf[..., :ncols] = s.view(SMR_NSEQ, SMR_SEQ, ncols)
    buf = buf.to(device)
    b0 = buf.clone()
    seq = SMR_SEQ if causal else None
    out = impl.softmax_rows(buf[..., :ncols], rows_per_seq=seq)
    assert out.data_ptr() == buf.data_ptr()
    assert torch.equal(buf[..., ncols:], b0[..., ncols:]), 'padding touched'
    got = buf[..., :ncols].contiguous()
    want = ref_softmax_rows(b0[..., :ncols], seq, torch.float64)
    ideal = ref_softmax_rows(b0[..., :ncols], seq, torch.float32).to(H)
    if causal:
        masked = torch.arange(ncols, device=device) > torch.arange(SMR_SEQ, device=device).view(SMR_SEQ, 1)
        assert float(got[:, masked].abs().max() if bool(masked.any()) else 0.0) == 0.0, 'a masked column is not an exact zero'
    fig = check(f"softmax_rows{'_causal' if causal else ''} ncols={ncols}", got, want, ideal)
    sum_got = float((got.double().sum(-1) - 1).abs().max())
    sum_ideal = float((ideal.double().sum(-1) - 1).abs().max())
    fig.update(rowsum_ideal=sum_ideal, rowsum_kernel=sum_got, rowsum_bound=2 * sum_ideal)
    assert sum_got <= 2 * sum_ideal, ('row sums', sum_got, sum_ideal)
    return fig


def expected_figures(with_huge=True):
    """how many entries a full pass over the tables leaves in FIGURES"""
    runs = [r for r in gn_runs() if with_huge or r[:5] != GN_HUGE[:5]]
    return (sum(2 if r[3] else 1 for r in runs) + len(LN_CASES) + len(SMB_CASES) + 2 * len(GEGLU_CASES) + 3 * len(ACT_SIZES)
            + len(POOL_CASES) + len(GATHER_C) + 1 + 2 * len(SMR_COLS))
