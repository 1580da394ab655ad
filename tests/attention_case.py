"""Shared by tests/test_attention_kernels_gpu.py (the HIP kernels) and tests/test_attention_case.py (the CPU stand-ins of
tests/host_emulation.py, the contract ideals, tiled restatements of the kernels and deliberate mutants of those): the case
tables of the attention kernels (videoswap_amd/csrc/attention.hip: flash, three temporal kernels; csrc/attention_bwd.hip: dQ,
dK / dV, delta; the materialised scores -> softmax -> PV path), fp64 references on fp16-exact inputs in plain PyTorch, the
ideals, and ONE comparison rule.  No kernels and no GPU calls of its own: every runner takes `impl` (videoswap_amd.ops or
host_emulation) and a device.

The rule is the one of tests/train_kernel_case.py (`measure`, imported, not copied): against `want` (float64),

    tensor rel-L2 <= 1.5 x the ideal's,  worst row <= 2 x,  max-abs <= 4 x,  every element inside its bound,  finite.

THE IDEAL is not the plain fp32 softmax but the kernels' documented arithmetic in plain fp32 PyTorch, rounded to fp16:
scores in fp32; P~ = exp2(s scale log2(e) - rowmax) ROUNDED TO FP16 before the second product; the denominator is the sum of
the rounded P~.  Backward: P and dS rounded to fp16 before their products.  Materialised path: the scaled scores are stored
in fp16 first, so its ideal is the stand-in chain of tests/host_emulation.py.

THE PER-ELEMENT BOUND is 1 fp16 ulp of `want` + 2^-10 of the row rms of `want` + the first-order effect of the fp16
roundings the contract names, taken twice (2^-11 relative -> 2^-10; half the subnormal spacing 2^-25 -> 2^-24), all
computed in fp64 from the inputs:

    o[q,c]    2^-10 sum_k p_qk |v_kc|      + 2^-24 sum_k |v_kc| / l_q,   l_q = sum_k exp(s_qk - max_q)
    dq[q,c]   2^-10 sum_k |dS_qk| |K_kc|   + 2^-24 sum_k |K_kc|
    dk[k,c]   2^-10 sum_q |dS_qk| |Q_qc|   + 2^-24 sum_q |Q_qc|
    dv[k,c]   2^-10 sum_q p_qk |dO_qc|     + 2^-24 sum_q |dO_qc|
    lse       |lse - want| <= 1.4427 2^-11 + 2^-20 max(1, |want|)   (a denominator of terms each within 2^-11 relative;
              16 fp32 ulps for s c - m and the log2), and exactly zero in [nq, round_up(nq, 64))
    probs of the materialised path: the fp16 rounding of the stored score s (|ds_j| <= 2^-11 |s_j|) moves p_k by
              p_k (ds_k - sum_j p_j ds_j): 2^-10 p_k (|s_k| + sum_j p_j |s_j|); its product with V adds
              sum_k (that + 2^-10 p_k + 2^-24) |v_kc|.
"""
import contextlib
import math

import torch

import train_kernel_case as tk
from train_kernel_case import H, _gen, _randn, measure, ulp16      # noqa: F401  (ulp16: re-exported for the tests)

LOG2E = 1.4426950408889634
FIGURES = []                    # one dict per compared tensor
SENTINEL = 1000.0
RULE = ('against fp64; ideal = the documented arithmetic in fp32 (P~ = exp2(s c - rowmax) rounded to fp16, denominator = sum '
        'of the rounded P~; backward: P and dS rounded to fp16; materialised path: scores stored in fp16) rounded to fp16: '
        'l2 <= 1.5 ideal, worst row <= 2 ideal, max-abs <= 4 ideal, per element <= 1 fp16 ulp + 2^-10 row rms + twice the '
        'first-order effect of the named fp16 roundings (elem_* are ratios to that bound); lse: |err| <= 1.4427 2^-11 + '
        '2^-20 max(1, |want|) (lse_* are ratios to that bound), zero padding exact; chained / materialised backward: the three '
        'whole-tensor metrics only')


# ------------------------------------------------------------------------------------------------
# the rule, bound to this file's FIGURES
# ------------------------------------------------------------------------------------------------
def check(name, got, want, ideal, elem_extra=None):
    """train_kernel_case.check, its figure moved into this file's FIGURES"""
    n = len(tk.FIGURES)
    try:
        return tk.check(name, got, want, ideal, elem_extra)
    finally:
        FIGURES.extend(tk.FIGURES[n:])
        del tk.FIGURES[n:]


def check_whole(name, got, want, ideal):
    """the three whole-tensor metrics (and finiteness) only"""
    fig, failed = measure(got, want, ideal)
    failed = [m for m in failed if m != 'elem']
    fig = dict(case=name, **{k: v for k, v in fig.items() if not k.startswith('elem')})
    print(' '.join(f'{k}={v:.3e}' if isinstance(v, float) else f'{k}={v}' for k, v in fig.items()))
    FIGURES.append(fig)
    assert not failed, (name, failed, fig)
    return fig


def check_lse(name, lse, want, ideal, nq):
    """lse [nb, heads, round_up(nq, 64)] fp32 against `want` [nb, heads, nq] fp64"""
    assert lse.dtype == torch.float32 and lse.shape == want.shape[:2] + ((nq + 63) // 64 * 64,), (lse.dtype, tuple(lse.shape))
    bound = LOG2E * 2.0 ** -11 + 2.0 ** -20 * want.abs().clamp_min(1.0)
    fig = {'case': name, 'lse_ideal': float(((ideal.double() - want).abs() / bound).max()),
           'lse_kernel': float(((lse[..., :nq].double() - want).abs() / bound).max()), 'lse_bound': 1.0,
           'lse_maxabs_kernel': float((lse[..., :nq].double() - want).abs().max()),
           'pad_zero': bool((lse[..., nq:] == 0).all()), 'finite': bool(torch.isfinite(lse).all())}
    failed = ([] if fig['lse_kernel'] <= 1.0 else ['lse']) + ([] if fig['pad_zero'] else ['lse_pad']) + \
        ([] if fig['finite'] else ['finite'])
    print(' '.join(f'{k}={v:.3e}' if isinstance(v, float) else f'{k}={v}' for k, v in fig.items()))
    FIGURES.append(fig)
    assert not failed, (name, failed, fig)
    return fig


@contextlib.contextmanager
def options(impl, opts):
    """kernel options for one call, restored to the defaults whatever happens"""
    try:
        for k, v in opts.items():
            impl.set_option(k, v)
        yield
    finally:
        for k in opts:
            impl.set_option(k, 0)


# ------------------------------------------------------------------------------------------------
# layouts
# ------------------------------------------------------------------------------------------------
def split(t, heads, dt):
    b, n, c = t.shape
    return t.to(dt).view(b, n, heads, c // heads).permute(0, 2, 1, 3)                      # [b, h, n, d]


def merge(t):
    b, h, n, d = t.shape
    return t.permute(0, 2, 1, 3).reshape(b, n, h * d)


def make_vt(v, ldvt=None):
    """[nkvb, nk, C] -> V^T [nkvb, C, ldvt >= round_up(nk, 8)], zero padded"""
    nkvb, nk, C = v.shape
    ld = ldvt or (nk + 7) // 8 * 8
    vt = torch.zeros(nkvb, C, ld, dtype=v.dtype, device=v.device)
    vt[:, :, :nk] = v.transpose(1, 2)
    return vt


def _coarse(g, *shape):
    """multiples of 1/8 within +-4: every fp32 (and fp64) sum of products of such values is exact in any order"""
    return ((torch.randn(*shape, generator=g) * 8).round().clamp(-32, 32) / 8).to(H)


# ------------------------------------------------------------------------------------------------
# flash forward: references
# ------------------------------------------------------------------------------------------------
def fwd_want(q, k, v, heads, scale, kv_div=1):
    """fp64 -> (out [nb, nq, C], lse [nb, heads, nq] (log2 domain), the per-element extra term, p)"""
    dt = torch.float64
    qh = split(q, heads, dt)
    kh, vh = (split(t, heads, dt).repeat_interleave(kv_div, 0) for t in (k, v))
    s = qh @ kh.transpose(-1, -2) * scale
    m = s.max(-1, keepdim=True).values
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    p = e / l
    lse = ((m + torch.log(l)) * LOG2E).squeeze(-1)
    extra = 2.0 ** -10 * (p @ vh.abs()) + 2.0 ** -24 * vh.abs().sum(-2, keepdim=True) / l
    return merge(p @ vh), lse, merge(extra), p


def fwd_ideal(q, k, v, heads, scale, kv_div=1):
    """the contract in fp32 -> (out fp16, lse fp32 [nb, heads, nq])"""
    dt = torch.float32
    qh = split(q, heads, dt)
    kh, vh = (split(t, heads, dt).repeat_interleave(kv_div, 0) for t in (k, v))
    t = (qh @ kh.transpose(-1, -2)) * (scale * LOG2E)
    m = t.max(-1, keepdim=True).values
    pt = torch.exp2(t - m).to(H).float()                     # P~ rounded to fp16 before the second product
    l = pt.sum(-1, keepdim=True)                             # the denominator: the sum of the ROUNDED P~
    return merge((pt @ vh) / l).to(H), (m + torch.log2(l)).squeeze(-1)


# ------------------------------------------------------------------------------------------------
# flash forward: cases.  A case is a dict; `fn` names the op ('attention' | 'attention_lse')
# ------------------------------------------------------------------------------------------------
def _fc(nq, nk, d=40, heads=2, nb=2, fn='attention', kind='randn', view=None, kv_div=1, opts=None):
    return dict(nq=nq, nk=nk, d=d, heads=heads, nb=nb, fn=fn, kind=kind, view=view, kv_div=kv_div, opts=opts or {})


FNS = ('attention', 'attention_lse')
HEAD_DIMS = (8, 16, 32, 40, 64, 80, 128, 160)
EDGE_NQ = (1, 32, 33, 127, 128, 129, 257)
EDGE_NK = (1, 8, 9, 63, 64, 65, 128, 129, 200)
# less than one query block / key tile, one short of / exactly / one past a tile, the 16-byte V^T granule (8, 9)
FLASH_EDGES = [_fc(nq, nk, fn=fn) for nq in EDGE_NQ for nk in EDGE_NK for fn in FNS]
# every head dim (both denominator routes: the ones row of the padded O^T tile, l_i on the VALU when d % 32 == 0) with one
# dominant key first (the max never grows again) or last (the max grows inside the masked partial tile)
FLASH_DIMS = [_fc(nq, nk, d=d, heads=3, fn='attention_lse', kind=kind)
              for d in HEAD_DIMS for nq, nk in ((33, 65), (129, 193)) for kind in ('dom0', 'domlast')]
VAR_NQ, VAR_NK = (1, 129, 257, 300), (65, 200)
FLASH_VARIANTS = (
    [_fc(nq, nk, d=d, fn=fn, opts={'attn_qb': qb}) for qb in (1, 2) for d in (40, 80) for nq in VAR_NQ for nk in VAR_NK for fn in FNS]
    + [_fc(nq, nk, d=40, opts={'attn_o16': 1}) for nq in VAR_NQ for nk in VAR_NK]
    # 64 queries per wave by the launch rule itself (d = 80, wg2 = 1 x 8 x 64 = 512, nq >= 256), with lse
    + [_fc(256, 65, d=80, heads=8, nb=64, fn='attention_lse')])
FLASH_VIEWS = (
    # q, k = the two column halves of one [nb, n, 2C] buffer (ldq = ldk = 2C): d = 40 reads 48-channel k-steps
    [_fc(n, n, d=d, fn=fn, view='halves') for d in (40, 80) for n in (65, 129) for fn in FNS]
    + [_fc(129, 77, d=40, nb=2 * kv, kv_div=kv, fn=fn) for kv in (2, 3) for fn in FNS]
    # explicit nk = 77 of k.shape[1] = 80, ldvt = 96: K rows >= nk and V^T columns >= 80 hold +-1000, [77, 80) zero
    + [_fc(129, 77, d=d, fn=fn, view='nk77') for d in (40, 80) for fn in FNS])
FLASH_KNOWN = (
    [_fc(33, nk, d=d, heads=2, kind='q0') for d in (40, 64) for nk in (1, 65, 200)]                    # the column mean of V
    + [_fc(33, nk, d=d, heads=2, kind='q0v1', fn=fn) for d in HEAD_DIMS for nk in (1, 65, 200) for fn in FNS])   # exactly 1.0
FLASH_RANGES = [_fc(129, 200, d=d, fn='attention_lse', kind=kind) for d in (40, 64) for kind in ('x4', 'samekeys')]
FLASH_TABLES = dict(edges=FLASH_EDGES, dims=FLASH_DIMS, variants=FLASH_VARIANTS, views=FLASH_VIEWS, known=FLASH_KNOWN,
                    ranges=FLASH_RANGES)


def flash_id(c):
    s = f"{c['fn']}-d{c['d']}-h{c['heads']}-nb{c['nb']}-{c['nq']}x{c['nk']}-{c['kind']}"
    s += f"-{c['view']}" if c['view'] else ''
    s += f"-kvdiv{c['kv_div']}" if c['kv_div'] != 1 else ''
    return s + ''.join(f'-{k}{v}' for k, v in c['opts'].items())


def flash_nfigs(c):
    return 2 if c['fn'] == 'attention_lse' else 1


def flash_inputs(c, device):
    """-> logical q, k, v (contiguous, what the references see) and the call's arguments (q, k, vt, nk)"""
    nb, heads, nq, nk, d, kind, kv = c['nb'], c['heads'], c['nq'], c['nk'], c['d'], c['kind'], c['kv_div']
    C = heads * d
    g = _gen(nb, heads, nq, nk, d, len(kind), kv)
    q, k, v = _randn(g, nb, nq, C), _randn(g, nb // kv, nk, C), _randn(g, nb // kv, nk, C)
    if kind in ('dom0', 'domlast'):
        # every query shares the direction (1, .., 1) per head; one key is 8 / sqrt(d) times it: its logit is 8 + N(0, 64 / d)
        q = (q.float() + 1.0).to(H)
        k[:, 0 if kind == 'dom0' else nk - 1] = 8.0 / math.sqrt(d)
    elif kind == 'x4':
        q, k = (q.float() * 4).to(H), (k.float() * 4).to(H)                 # logit std ~ 16
    elif kind == 'samekeys':
        k = k[:, :1].expand(-1, nk, -1).contiguous()                        # exactly uniform
    elif kind in ('q0', 'q0v1'):
        q = torch.zeros_like(q)
        if kind == 'q0v1':
            v = torch.ones_like(v)
    q, k, v = q.to(device), k.to(device), v.to(device)
    qa, ka, vta, nka = q, k, make_vt(v), None
    if c['view'] == 'halves':
        assert nq == nk and kv == 1
        buf = torch.cat([q, k], dim=-1)
        qa, ka = buf[..., :C], buf[..., C:]
    elif c['view'] == 'nk77':
        assert nk == 77
        ka = torch.full((nb // kv, 80, C), SENTINEL, dtype=H, device=device)
        ka[:, 1::2] = -SENTINEL
        ka[:, :nk] = k
        vta = torch.full((nb // kv, C, 96), SENTINEL, dtype=H, device=device)
        vta[:, :, 1::2] = -SENTINEL
        vta[:, :, :80] = make_vt(v)
        nka = nk
    return (q, k, v), (qa, ka, vta, nka)


def run_flash(impl, device, c, fn=None):
    """`fn`: replaces impl.attention / impl.attention_lse (restatements and mutants of tests/test_attention_case.py)"""
    (q, k, v), (qa, ka, vta, nka) = flash_inputs(c, device)
    heads, nq, kv = c['heads'], c['nq'], c['kv_div']
    scale = c['d'] ** -0.5
    with options(impl, c['opts']) if c['opts'] else contextlib.nullcontext():
        res = (fn or getattr(impl, c['fn']))(qa, ka, vta, heads, scale, kv_div=kv, nk=nka)
    out, lse = res if c['fn'] == 'attention_lse' else (res, None)
    want, want_lse, extra, _ = fwd_want(q, k, v, heads, scale, kv)
    ideal, ideal_lse = fwd_ideal(q, k, v, heads, scale, kv)
    name = 'flash ' + flash_id(c)
    assert out.shape == want.shape and out.is_contiguous()
    if c['kind'] == 'q0v1':
        assert torch.equal(out, torch.ones_like(out)), (name, ['exactly_one'],                    # softmax(0) @ 1 = 1.0
                                                       {'maxabs_kernel': float((out.float() - 1).abs().max())})
    figs = [check(name + ' out', out, want, ideal, elem_extra=extra)]
    if lse is not None:
        figs.append(check_lse(name + ' lse', lse, want_lse, ideal_lse, nq))
    return figs


# ------------------------------------------------------------------------------------------------
# flash backward
# ------------------------------------------------------------------------------------------------
def bwd_want(q, k, v, out, dout, lse, heads, scale, kv_div=1):
    """fp64 evaluation of the kernel's function of ITS inputs: P = exp2(s c - lse), delta = dO . out
    -> (dq, dk, dv, their per-element extra terms); with kv_div > 1 only dq means anything (the kernel gives no dk / dv)"""
    dt = torch.float64
    qh, oh, gh = split(q, heads, dt), split(out, heads, dt), split(dout, heads, dt)
    kh, vh = (split(t, heads, dt).repeat_interleave(kv_div, 0) for t in (k, v))
    nq = q.shape[1]
    p = torch.exp2(qh @ kh.transpose(-1, -2) * (scale * LOG2E) - lse[..., :nq, None].to(dt))
    delta = (gh * oh).sum(-1, keepdim=True)
    ds = scale * p * (gh @ vh.transpose(-1, -2) - delta)
    dq, dk, dv = ds @ kh, ds.transpose(-1, -2) @ qh, p.transpose(-1, -2) @ gh
    a = ds.abs()
    xq = 2.0 ** -10 * (a @ kh.abs()) + 2.0 ** -24 * kh.abs().sum(-2, keepdim=True)
    xk = 2.0 ** -10 * (a.transpose(-1, -2) @ qh.abs()) + 2.0 ** -24 * qh.abs().sum(-2, keepdim=True)
    xv = 2.0 ** -10 * (p.transpose(-1, -2) @ gh.abs()) + 2.0 ** -24 * gh.abs().sum(-2, keepdim=True)
    return tuple(merge(t).contiguous() for t in (dq, dk, dv, xq, xk, xv))


def bwd_ideal(q, k, v, out, dout, lse, heads, scale, kv_div=1):
    """the contract in fp32: P and dS rounded to fp16 before their products -> (dq, dk, dv) fp16"""
    dt = torch.float32
    qh, oh, gh = split(q, heads, dt), split(out, heads, dt), split(dout, heads, dt)
    kh, vh = (split(t, heads, dt).repeat_interleave(kv_div, 0) for t in (k, v))
    nq = q.shape[1]
    p = torch.exp2(qh @ kh.transpose(-1, -2) * (scale * LOG2E) - lse[..., :nq, None].to(dt))
    delta = (gh * oh).sum(-1, keepdim=True)
    ds = (scale * p * (gh @ vh.transpose(-1, -2) - delta)).to(H).float()
    p16 = p.to(H).float()
    return tuple(merge(t).to(H).contiguous() for t in (ds @ kh, ds.transpose(-1, -2) @ qh, p16.transpose(-1, -2) @ gh))


def autograd_want(q, k, v, dout, heads, scale):
    """true fp64 autograd of softmax(scale Q K^T) V"""
    qr, kr, vr = (t.double().requires_grad_(True) for t in (q, k, v))
    with torch.enable_grad():
        qh, kh, vh = (split(t, heads, torch.float64) for t in (qr, kr, vr))
        o = merge(torch.softmax(qh @ kh.transpose(-1, -2) * scale, -1) @ vh)
        return torch.autograd.grad(o, (qr, kr, vr), dout.double())


def _bc(nq, nk, d=40, heads=2, nb=2, kv_div=1, chained=False):
    return dict(nq=nq, nk=nk, d=d, heads=heads, nb=nb, kv_div=kv_div, chained=chained)


BWD_NQ = (1, 63, 64, 65, 127, 128, 129, 200)
BWD_NK = (1, 8, 9, 63, 64, 65, 127, 128, 129, 200)
BWD_CASES = ([_bc(nq, nk) for nq in BWD_NQ for nk in BWD_NK]
             + [_bc(nq, nk, d=d) for d in (64, 80) for nq, nk in ((1, 1), (65, 129), (129, 65), (200, 200))]
             + [_bc(129, 77, nb=4, kv_div=2)])                                       # shared text keys: dq only
BWD_CHAINED = [_bc(129, 200, d=d, chained=True) for d in (40, 64, 80)]               # the kernel's own forward feeds the backward


def bwd_id(c):
    return f"d{c['d']}-{c['nq']}x{c['nk']}" + (f"-kvdiv{c['kv_div']}" if c['kv_div'] != 1 else '') + ('-chained' if c['chained'] else '')


def bwd_nfigs(c):
    return 1 if c['kv_div'] != 1 else 3


def bwd_inputs(c, device):
    nb, heads, nq, nk, d, kv = c['nb'], c['heads'], c['nq'], c['nk'], c['d'], c['kv_div']
    C = heads * d
    g = _gen(nb, heads, nq, nk, d, kv, 7)
    if nk == 1:
        # one key: P = 1, and dS = scale (dP - delta) is an exact zero only if dP = dO . V and delta = dO . O (O = V) cancel
        # exactly.  On a coarse grid every fp32 sum is exact in any order; with N(0, 1) inputs the case would compare the
        # rounding noise of one summation order with that of another
        q, k, v, dout = _coarse(g, nb, nq, C), _coarse(g, nb // kv, nk, C), _coarse(g, nb // kv, nk, C), _coarse(g, nb, nq, C)
    else:
        q, k, v, dout = _randn(g, nb, nq, C), _randn(g, nb // kv, nk, C), _randn(g, nb // kv, nk, C), _randn(g, nb, nq, C)
        # a peaked (saturated) row: query 0 on the last key, logit 2 |q|^2 / sqrt(d) ~ 2 sqrt(d); the other P of the row
        # underflow into the fp16 subnormals.  There P = 1 meets dP - delta, a difference of two fp32 sums of size |dO| |V|
        # whose true value is near zero, and its fp32 noise (~ 1e-6 |dO| |V|) is multiplied by that key's own large K.  The
        # bound has a term for every fp16 rounding and none for fp32 accumulation, so the row's dO is scaled by 1 / 8 (exact
        # in fp16): measured on the ideal at 1 x 8, the noise is then 0.3 of the 2^-24 sum |K| term instead of 2.5 times it
        k[:, nk - 1] = (q[::kv, 0].float() * 2).to(H)
        dout[:, 0] = (dout[:, 0].float() / 8).to(H)
    return tuple(t.to(device) for t in (q, k, v, dout))


def run_bwd(impl, device, c, fn=None, fwd=None):
    """fn: replaces impl.attention_bwd; fwd: replaces impl.attention_lse (the chained cases)"""
    q, k, v, dout = bwd_inputs(c, device)
    heads, nq, kv = c['heads'], c['nq'], c['kv_div']
    scale = c['d'] ** -0.5
    need_kv = kv == 1
    name = 'attention_bwd ' + bwd_id(c)
    bwd = fn or impl.attention_bwd
    if c['chained']:
        out, lse = (fwd or impl.attention_lse)(q, k, make_vt(v), heads, scale)
        got = bwd(q, k, v, out, dout, lse, heads, scale, kv_div=kv, need_kv=need_kv)
        want = autograd_want(q, k, v, dout, heads, scale)
        iout, ilse = fwd_ideal(q, k, v, heads, scale)
        ideal = bwd_ideal(q, k, v, iout, dout, ilse, heads, scale)
        return [check_whole(f'{name} {n}', g_, w.contiguous(), i) for n, g_, w, i in zip(('dq', 'dk', 'dv'), got, want, ideal)]
    # on its own: the reference's out (rounded to fp16) and lse (rounded to fp32, zero padded) are the kernel's inputs, so the
    # fp16 rounding of `out` inside delta is not charged to the kernel
    wout, wlse, _, _ = fwd_want(q, k, v, heads, scale, kv)
    out = wout.to(H)
    lse = torch.zeros(q.shape[0], heads, (nq + 63) // 64 * 64, dtype=torch.float32, device=q.device)
    lse[..., :nq] = wlse.float()
    got = bwd(q, k, v, out, dout, lse, heads, scale, kv_div=kv, need_kv=need_kv)
    wdq, wdk, wdv, xq, xk, xv = bwd_want(q, k, v, out, dout, lse, heads, scale, kv)
    idq, idk, idv = bwd_ideal(q, k, v, out, dout, lse, heads, scale, kv)
    figs = [check(name + ' dq', got[0], wdq, idq, elem_extra=xq)]
    if need_kv:
        figs.append(check(name + ' dk', got[1], wdk, idk, elem_extra=xk))
        figs.append(check(name + ' dv', got[2], wdv, idv, elem_extra=xv))
    else:
        assert got[1] is None and got[2] is None
    return figs


# ------------------------------------------------------------------------------------------------
# temporal attention: q [(b fq s), C], k / v [(b fk s), C]
# ------------------------------------------------------------------------------------------------
def _sites(t, B, f, hw, heads, dt):
    return t.to(dt).reshape(B, f, hw, heads, -1).permute(0, 2, 3, 1, 4)                   # [b, s, h, f, d]


def _rows(o):
    B, hw, heads, f, d = o.shape
    return o.permute(0, 3, 1, 2, 4).reshape(B * f * hw, heads * d)


def temporal_want(q, k, v, B, fq, fk, hw, heads, scale):
    dt = torch.float64
    qs, ks, vs = _sites(q, B, fq, hw, heads, dt), _sites(k, B, fk, hw, heads, dt), _sites(v, B, fk, hw, heads, dt)
    s = qs @ ks.transpose(-1, -2) * scale
    e = torch.exp(s - s.max(-1, keepdim=True).values)
    l = e.sum(-1, keepdim=True)
    p = e / l
    extra = 2.0 ** -10 * (p @ vs.abs()) + 2.0 ** -24 * vs.abs().sum(-2, keepdim=True) / l
    return _rows(p @ vs).contiguous(), _rows(extra).contiguous()


def temporal_ideal(q, k, v, B, fq, fk, hw, heads, scale):
    dt = torch.float32
    qs, ks, vs = _sites(q, B, fq, hw, heads, dt), _sites(k, B, fk, hw, heads, dt), _sites(v, B, fk, hw, heads, dt)
    t = (qs @ ks.transpose(-1, -2)) * (scale * LOG2E)
    pt = torch.exp2(t - t.max(-1, keepdim=True).values).to(H).float()
    return _rows((pt @ vs) / pt.sum(-1, keepdim=True)).to(H).contiguous()


def _tc(fq, fk, d, heads=8, hw=3, B=1, out=0, view=None, scale=None):
    return dict(fq=fq, fk=fk, d=d, heads=heads, hw=hw, B=B, out=out, view=view, scale=scale)


T_DIMS = (40, 80, 160)
T_PACKED_FRAMES = ((1, 1), (3, 3), (5, 16), (16, 5), (12, 32), (17, 17), (32, 32))
# the matrix-core kernel: G = 32 / max(fq, fk) heads per tile, fq != fk, frame counts that do not divide 32, one frame, one
# site, head counts that leave the last group (5 of 2, 6 or 10 per tile) or the last wave (1, 5) partly empty
T_PACKED = [_tc(fq, fk, d, heads=h, hw=hw, B=B, out=o) for fq, fk in T_PACKED_FRAMES for d in T_DIMS for h in (1, 5, 8)
            for hw in (1, 3) for B in (1, 2) for o in (0, 1)]
T_LONG = [_tc(fq, fk, d, heads=5, hw=3, B=B, out=o) for fq in (1, 7, 32) for fk in (33, 65, 127, 128) for d in T_DIMS
          for B in (1, 2) for o in (0, 1)]
T_OTHER = (
    [_tc(7, 129, 40, heads=5, B=B, out=o) for B in (1, 2) for o in (0, 1)]                  # the VALU kernel at a UNet head dim
    + [_tc(6, 9, 24, heads=3, B=B, out=o) for B in (1, 2) for o in (0, 1)]                  # and at a head dim with no MFMA form
    + [_tc(fq, fk, d, heads=5, B=B, out=o) for fq, fk in ((33, 33), (40, 64)) for d in T_DIMS for B in (1, 2) for o in (0, 1)]
    + [_tc(fq, fk, d, heads=5, B=2, view='fused') for fq, fk, d in ((5, 16, 40), (17, 17, 80), (7, 65, 160), (6, 9, 24))]
    # the temporal kernels scale BEFORE the row max: any finite scale is legal there
    + [_tc(fq, fk, d, heads=5, B=2, scale=sc) for fq, fk, d in ((5, 16, 40), (7, 33, 40), (6, 9, 24)) for sc in (0.0, -1.0)])
TEMPORAL_TABLES = dict(packed=T_PACKED, long=T_LONG, other=T_OTHER)
TEMPORAL_LDS_REFUSAL = _tc(64, 200, 160, heads=1, hw=1)


def temporal_id(c):
    s = f"{c['fq']}x{c['fk']}-d{c['d']}-h{c['heads']}-hw{c['hw']}-B{c['B']}-out{c['out']}"
    s += f"-{c['view']}" if c['view'] else ''
    return s + (f"-scale{c['scale']:g}" if c['scale'] is not None else '')


def temporal_inputs(c, device):
    B, fq, fk, hw, heads, d = c['B'], c['fq'], c['fk'], c['hw'], c['heads'], c['d']
    C = heads * d
    g = _gen(B, fq, fk, hw, heads, d)
    q, k, v = _randn(g, B * fq * hw, C), _randn(g, B * fk * hw, C), _randn(g, B * fk * hw, C)
    if c['view'] == 'fused':                     # column slices of one [rows, 3C] buffer (rows: the larger of the two counts)
        rows = max(q.shape[0], k.shape[0])
        buf = _randn(g, rows, 3 * C).to(device)
        buf[:q.shape[0], :C], buf[:k.shape[0], C:2 * C], buf[:k.shape[0], 2 * C:] = q.to(device), k.to(device), v.to(device)
        return buf[:q.shape[0], :C], buf[:k.shape[0], C:2 * C], buf[:k.shape[0], 2 * C:]
    return q.to(device), k.to(device), v.to(device)


def run_temporal(impl, device, c, fn=None):
    B, fq, fk, hw, heads, d = c['B'], c['fq'], c['fk'], c['hw'], c['heads'], c['d']
    q, k, v = temporal_inputs(c, device)
    scale = d ** -0.5 if c['scale'] is None else c['scale'] * d ** -0.5
    with options(impl, {'temporal_out': c['out']}):
        out = (fn or impl.temporal_attention)(q, k, v, B, fq, fk, hw, heads, scale)
    want, extra = temporal_want(q, k, v, B, fq, fk, hw, heads, scale)
    assert out.shape == want.shape and out.is_contiguous()
    return [check('temporal ' + temporal_id(c), out, want, temporal_ideal(q, k, v, B, fq, fk, hw, heads, scale), elem_extra=extra)]


# ------------------------------------------------------------------------------------------------
# the materialised path: attention_scores -> (softmax_rows) -> attention_pv, and autograd._attention_backward
# ------------------------------------------------------------------------------------------------
def _mc(nq, nk, d, mode, nb=2, kv_div=1):
    return dict(nq=nq, nk=nk, d=d, mode=mode, nb=nb, kv_div=kv_div, heads=8)


MAT_SHAPES = ((1, 1), (3, 5), (16, 16), (24, 24), (16, 77))
MAT_CASES = ([_mc(nq, nk, d, mode) for nq, nk in MAT_SHAPES for d in (40, 160) for mode in ('softmax', 'raw', 'causal')]
             + [_mc(16, 16, 40, 'softmax', nb=300)]                                   # the batched grid
             + [_mc(16, 77, d, 'softmax', nb=4, kv_div=2) for d in (40, 160)])
MAT_BWD_CASES = [_mc(16, 16, 40, 'bwd', nb=1024), _mc(16, 16, 160, 'bwd', nb=1024), _mc(3, 5, 40, 'bwd', nb=3),
                 _mc(3, 5, 160, 'bwd', nb=3)]


def mat_id(c):
    return f"{c['mode']}-d{c['d']}-{c['nq']}x{c['nk']}-nb{c['nb']}" + (f"-kvdiv{c['kv_div']}" if c['kv_div'] != 1 else '')


def mat_nfigs(c):
    return {'softmax': 2, 'causal': 2, 'raw': 1, 'bwd': 3}[c['mode']]


def mat_inputs(c, device):
    nb, heads, nq, nk, d, kv = c['nb'], c['heads'], c['nq'], c['nk'], c['d'], c['kv_div']
    C = heads * d
    g = _gen(nb, nq, nk, d, kv, 11)
    return tuple(t.to(device) for t in (_randn(g, nb, nq, C), _randn(g, nb // kv, nk, C), _randn(g, nb // kv, nk, C),
                                        _randn(g, nb, nq, C)))


def run_materialised(impl, device, c):
    import host_emulation
    q, k, v, _ = mat_inputs(c, device)
    heads, nq, nk, kv, mode = c['heads'], c['nq'], c['nk'], c['kv_div'], c['mode']
    scale = c['d'] ** -0.5
    causal, softmax = mode == 'causal', mode != 'raw'
    name = 'materialised ' + mat_id(c)
    probs = impl.attention_scores(q, k, heads, scale, kv_div=kv, causal=causal, softmax=softmax)
    assert probs.shape == (c['nb'], heads, nq, nk)
    with torch.no_grad():
        iprobs = host_emulation.attention_scores(q.cpu(), k.cpu(), heads, scale, kv_div=kv, causal=causal, softmax=softmax)
    dt = torch.float64
    qh = split(q, heads, dt)
    kh, vh = (split(t, heads, dt).repeat_interleave(kv, 0) for t in (k, v))
    s = qh @ kh.transpose(-1, -2) * scale
    if not softmax:
        return [check(name + ' scores', probs.contiguous(), s, iprobs.to(device))]
    sm = s.masked_fill(torch.ones(nq, nk, dtype=torch.bool, device=s.device).triu(1), float('-inf')) if causal else s
    p = sm.softmax(-1)
    if causal:
        assert float(probs.masked_select(torch.ones(nq, nk, dtype=torch.bool, device=s.device).triu(1)).abs().sum()) == 0.0
    xp = 2.0 ** -10 * p * (s.abs() + (p * s.abs()).sum(-1, keepdim=True))
    figs = [check(name + ' probs', probs.contiguous(), p, iprobs.to(device), elem_extra=xp)]
    vt = make_vt(v)
    out = impl.attention_pv(probs, vt, kv_div=kv)
    with torch.no_grad():
        iout = host_emulation.attention_pv(iprobs, vt.cpu(), kv_div=kv)
    xo = merge((xp + 2.0 ** -10 * p + 2.0 ** -24) @ vh.abs())
    figs.append(check(name + ' out', out, merge(p @ vh).contiguous(), iout.to(device), elem_extra=xo))
    return figs


def run_materialised_bwd(backward, device, c):
    """`backward`: videoswap_amd.autograd._attention_backward with the implementation under test installed.  Against fp64
    autograd by the three whole-tensor metrics; the ideal is the same function over the stand-ins of host_emulation."""
    import host_emulation
    from videoswap_amd import autograd as vsx_autograd
    q, k, v, dout = mat_inputs(c, device)
    heads = c['heads']
    scale = c['d'] ** -0.5
    got = backward(q, k, v, dout, heads, scale, 1, True)
    with host_emulation.installed(), torch.no_grad():
        ideal = vsx_autograd._attention_backward(q.cpu(), k.cpu(), v.cpu(), dout.cpu(), heads, scale, 1, True)
    want = autograd_want(q, k, v, dout, heads, scale)
    name = 'materialised ' + mat_id(c)
    return [check_whole(f'{name} {n}', g_.contiguous(), w.contiguous(), i.to(device).contiguous())
            for n, g_, w, i in zip(('dq', 'dk', 'dv'), got, want, ideal)]


def expected_figures():
    """how many entries a full pass over the tables leaves in FIGURES"""
    return (sum(flash_nfigs(c) for t in FLASH_TABLES.values() for c in t) + sum(bwd_nfigs(c) for c in BWD_CASES + BWD_CHAINED)
            + sum(len(t) for t in TEMPORAL_TABLES.values()) + sum(mat_nfigs(c) for c in MAT_CASES + MAT_BWD_CASES))


def summarise(figures):
    """one record per group (the GPU test that left the figures): how many tensors, and per metric the tensor that came closest
    to its bound - as a fraction of the bound, with the kernel's and the ideal's figure and the case"""
    r4 = (lambda v: float(f'{v:.4g}'))
    groups = {}
    for fig in figures:
        groups.setdefault(fig.get('group', ''), []).append(fig)
    out = []
    for name, figs in groups.items():
        rec = {'group': name, 'tensors': len(figs), 'all_finite': all(f['finite'] for f in figs)}
        for m in ('l2', 'row', 'maxabs', 'elem', 'lse'):
            worst = None
            for f in figs:
                if m + '_kernel' in f:
                    k, b = f[m + '_kernel'], f[m + '_bound']
                    frac = k / b if b > 0 else (0.0 if k == 0 else float('inf'))
                    if worst is None or frac > worst[0]:
                        worst = (frac, k, f[m + '_ideal'], f['case'])
            if worst is not None:
                rec[m] = {'of_bound': r4(worst[0]), 'kernel': r4(worst[1]), 'ideal': r4(worst[2]), 'case': worst[3]}
        out.append(rec)
    return out
