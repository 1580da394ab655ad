"""The comparison rule and the case tables of tests/attention_case.py, proven on the CPU before a GPU sees them.

1. Every case of the GPU tables (tests/test_attention_kernels_gpu.py) runs three things through the rule, and all stay inside
   every bound: the stand-ins of tests/host_emulation.py, the contract ideals themselves, and a tiled restatement of each
   kernel's structure in fp32 PyTorch (64-key / 64-query tiles with a running max and a late rescale; packed heads with a
   block-diagonal mask for the temporal matrix-core kernel; 32-key blocks for its long form).
2. Deliberate mutants of those restatements - the index, mask and rescale mistakes a kernel of this kind can make and a
   whole-tensor rel-L2 of 3e-3 lets through - are each REJECTED by the rule; unmutated, the same restatement passes (part 1).
   A mutant that passes means the rule or the case table is too loose.
"""

import pytest
import torch
import torch.nn.functional as F

import attention_case as ac
import host_emulation
from attention_case import H, LOG2E, merge, split

CPU = 'cpu'
LEFT_OUT = []          # cases too large for the CPU would be named here (none are); the cap is asserted below


# ------------------------------------------------------------------------------------------------
# the contract ideals and the tiled restatements, each with the call signatures of videoswap_amd.ops
# ------------------------------------------------------------------------------------------------
def _kv(k, vt, nk):
    nk = k.shape[1] if nk is None else nk
    return nk, k[:, :nk], vt[:, :, :nk].transpose(1, 2)


def _lse_buf(lse, nq):
    buf = torch.zeros(*lse.shape[:2], (nq + 63) // 64 * 64)
    buf[..., :nq] = lse
    return buf


class Ideal:
    """the contract ideals of attention_case.py in the kernels' place"""
    set_option = staticmethod(lambda name, value: None)

    @staticmethod
    def attention(q, k, vt, heads, scale, kv_div=1, nk=None):
        nk, k, v = _kv(k, vt, nk)
        return ac.fwd_ideal(q, k, v, heads, scale, kv_div)[0]

    @staticmethod
    def attention_lse(q, k, vt, heads, scale, kv_div=1, nk=None):
        nk, k, v = _kv(k, vt, nk)
        out, lse = ac.fwd_ideal(q, k, v, heads, scale, kv_div)
        return out, _lse_buf(lse, q.shape[1])

    @staticmethod
    def attention_bwd(q, k, v, out, dout, lse, heads, scale, kv_div=1, need_kv=True):
        dq, dk, dv = ac.bwd_ideal(q, k, v, out, dout, lse, heads, scale, kv_div)
        return (dq, dk, dv) if need_kv else (dq, None, None)

    temporal_attention = staticmethod(ac.temporal_ideal)


def _wide_heads(t, heads, d, w):
    """[b, h, n, w] with w > d channels per head read from the view's underlying buffer: what a k-step that is not kept
    inside the head reads (the next head's columns, the other half of a fused projection, the next row)"""
    base = t._base if t._base is not None else t
    flat = torch.cat([base.reshape(-1), base.new_zeros(w)])
    b, n, _ = t.shape
    x = torch.as_strided(flat, (b, n, heads, w), (t.stride(0), t.stride(1), d, 1), t.storage_offset() - base.storage_offset())
    return x.float().permute(0, 2, 1, 3)


def flash_tiled(q, k, vt, heads, scale, kv_div=1, nk=None, mutant=None):
    """flash_attn_kernel restated in fp32: 64-key tiles, the row max taken BEFORE scaling, running max m, O (and l) rescaled
    when it grows, P~ = exp2(s c - m) rounded to fp16 for the second product, keys past nk masked in the last tile only, the
    denominator from the rounded P~ (the ones row of the padded O^T tile) or, when d % 32 == 0, from the fp32 P~ (l_i on the
    VALU).  K rows / V^T columns past the end read as zero, as through the buffer descriptor.  -> (out, lse buffer)"""
    nb, nq, C = q.shape
    d = C // heads
    nk = k.shape[1] if nk is None else nk
    c = scale * LOG2E
    if mutant == 'wide_qk':
        qh, kh = _wide_heads(q, heads, d, 48), _wide_heads(k, heads, d, 48)
    else:
        qh, kh = split(q, heads, torch.float32), split(k, heads, torch.float32)
    ntile = (nk + 63) // 64
    kh = F.pad(kh[:, :, :nk], (0, 0, 0, ntile * 64 - nk)).repeat_interleave(kv_div, 0)
    vth = vt.float().view(vt.shape[0], heads, d, vt.shape[2])
    vth = (F.pad(vth, (0, ntile * 64 - vt.shape[2])) if vt.shape[2] < ntile * 64 else vth).repeat_interleave(kv_div, 0)
    m = torch.full((nb, heads, nq, 1), float('-inf'))
    l = torch.zeros(nb, heads, nq, 1)
    o = torch.zeros(nb, heads, nq, d)
    lim = nk + (mutant == 'count_pad') - (mutant == 'drop_last')
    for j0 in range(0, nk, 64):
        last = j0 + 64 >= nk
        s = qh @ kh[:, :, j0:j0 + 64].transpose(-1, -2)
        if j0 + 64 > lim or mutant == 'drop_last':
            s = s.masked_fill(j0 + torch.arange(64) >= lim, float('-inf'))
        m_new = torch.maximum(m, s.max(-1, keepdim=True).values * c)
        alpha = torch.exp2(m - m_new)
        if not (mutant == 'no_o_rescale' and last):
            o = o * alpha
        if not (mutant == 'no_l_rescale' and last):
            l = l * alpha
        e = torch.exp2(s * c - m_new)
        p16 = e.to(H).float()
        l = l + (p16 if d % 32 else e).sum(-1, keepdim=True)
        o = o + p16 @ vth[..., j0:j0 + 64].transpose(-1, -2)
        m = m_new
    out = merge(o / l).to(H).contiguous()
    lse = (torch.log2(l) if mutant == 'lse_nomax' else m + torch.log2(l)).squeeze(-1) + (2e-3 if mutant == 'lse_off' else 0.0)
    if mutant == 'q128_from_q0':
        out[:, 128] = out[:, 0]
    return out, _lse_buf(lse, nq)


def bwd_tiled(q, k, v, out, dout, lse, heads, scale, kv_div=1, need_kv=True, mutant=None):
    """attn_delta_kernel, attn_bwd_dq_kernel (key tiles of 64, keys past nk masked to P = 0) and attn_bwd_dkv_kernel (query
    tiles of 64; a query past the end has Q = dO = 0 and zero statistics) restated in fp32; P and dS rounded to fp16 for the
    second products"""
    nb, nq, C = q.shape
    nk = k.shape[1]
    d = C // heads
    f32 = torch.float32
    qh, oh, gh = split(q, heads, f32), split(out, heads, f32), split(dout, heads, f32)
    kh, vh = (split(t, heads, f32).repeat_interleave(kv_div, 0) for t in (k, v))
    c = scale * LOG2E
    nd = d // 2 if mutant == 'delta_half' else d
    delta = (gh[..., :nd] * oh[..., :nd]).sum(-1, keepdim=True)
    L = lse[..., :nq, None].float()
    sc = 1.0 if mutant == 'no_scale' else scale
    dq = torch.zeros_like(qh)
    lim = nk + (mutant == 'dq_pad_unmasked')
    for j0 in range(0, nk, 64):
        pad = (0, 0, 0, max(0, j0 + 64 - nk))
        kt, vt_ = F.pad(kh[:, :, j0:j0 + 64], pad), F.pad(vh[:, :, j0:j0 + 64], pad)
        p = torch.exp2(qh @ kt.transpose(-1, -2) * c - L).masked_fill(j0 + torch.arange(64) >= lim, 0.0)
        ds = (p * (gh @ vt_.transpose(-1, -2) - delta) * sc).to(H).float()
        dq = dq + ds @ kt
    back = (lambda t: merge(t).to(H).contiguous())
    if not need_kv:
        return back(dq), None, None
    dk, dv = torch.zeros_like(kh), torch.zeros_like(vh)
    for j0 in range(0, nq, 64):
        if mutant == 'drop_q64' and j0 == 64:
            continue
        pad = (0, 0, 0, max(0, j0 + 64 - nq))
        qt, gt = F.pad(qh[:, :, j0:j0 + 64], pad), F.pad(gh[:, :, j0:j0 + 64], pad)
        Lt, dt_ = F.pad(L[:, :, j0:j0 + 64], pad), F.pad(delta[:, :, j0:j0 + 64], pad)
        p = torch.exp2(qt @ kh.transpose(-1, -2) * c - Lt)
        ds = p * (gt @ vh.transpose(-1, -2) - dt_) * sc
        dv = dv + p.to(H).float().transpose(-1, -2) @ gt
        dk = dk + ds.to(H).float().transpose(-1, -2) @ qt
    return back(dq), back(dk), back(dv)


def temporal_packed(q, k, v, B, fq, fk, hw, heads, scale, mutant=None):
    """temporal_attn_mfma_kernel restated: G = 32 / max(fq, fk) consecutive heads of a site packed along both dimensions of
    one 32 x 32 tile S[(g', query), (g, key)], everything but the diagonal blocks and the padding masked to -inf, the scores
    scaled BEFORE the row max, P rounded to fp16 for the second product, the denominator from the fp32 P"""
    C = q.shape[-1]
    d = C // heads
    G = 32 // max(fq, fk)
    ng = (heads + G - 1) // G

    def pack(t, f):                    # [(b f s), C] -> [B, hw, ng, 32, d]: row g * f + frame of group ng, zero padded
        x = F.pad(t.float().reshape(B, f, hw, heads, d), (0, 0, 0, ng * G - heads))
        x = x.reshape(B, f, hw, ng, G, d).permute(0, 2, 3, 4, 1, 5).reshape(B, hw, ng, G * f, d)
        return F.pad(x, (0, 0, 0, 32 - G * f))
    Qp, Kp, Vp = pack(q, fq), pack(k, fk), pack(v, fk)
    S = Qp @ Kp.transpose(-1, -2)                                      # [B, hw, ng, 32 query columns, 32 keys]
    idx = torch.arange(32)
    qg, kg = idx // fq, idx // fk
    head_ok = (torch.arange(ng)[:, None] * G + torch.arange(G)[None, :]) < heads          # [ng, G]
    qok = (qg < G)[None, :] & head_ok[:, qg.clamp(max=G - 1)]                             # [ng, 32]
    kok = (kg < G)[None, :] & head_ok[:, kg.clamp(max=G - 1)]
    valid = qok[:, :, None] & (kg[None, None, :] == qg[None, :, None]) & (idx < G * fk)[None, None, :]
    if mutant == 'offdiag':
        valid = qok[:, :, None] & kok[:, None, :]
    elif mutant == 'padkeys':
        valid = valid | (qok[:, :, None] & (idx >= G * fk)[None, None, :])
    s = torch.where(valid, S * (scale * LOG2E), torch.tensor(float('-inf')))
    mx = s.max(-1, keepdim=True).values
    mx = torch.where(torch.isinf(mx), torch.zeros_like(mx), mx)
    e = torch.exp2(s - mx)
    tot = e.sum(-1, keepdim=True)
    o = (e.to(H).float() @ Vp) * torch.where(tot > 0, 1.0 / tot, torch.zeros_like(tot))
    o = o[:, :, :, :G * fq].reshape(B, hw, ng * G, fq, d)[:, :, :heads]
    return ac._rows(o).to(H).contiguous()


def temporal_long(q, k, v, B, fq, fk, hw, heads, scale):
    """temporal_attn_mfma_long_kernel: the softmax over all fk score registers, the second product in blocks of 32 keys"""
    f32 = torch.float32
    qs, ks, vs = ac._sites(q, B, fq, hw, heads, f32), ac._sites(k, B, fk, hw, heads, f32), ac._sites(v, B, fk, hw, heads, f32)
    s = (qs @ ks.transpose(-1, -2)) * (scale * LOG2E)
    e = torch.exp2(s - s.max(-1, keepdim=True).values)
    o = sum(e[..., kb:kb + 32].to(H).float() @ vs[..., kb:kb + 32, :] for kb in range(0, fk, 32))
    return ac._rows(o * (1.0 / e.sum(-1, keepdim=True))).to(H).contiguous()


def temporal_valu(q, k, v, B, fq, fk, hw, heads, scale):
    """temporal_attn_kernel: fp32 probabilities, normalised before the second product"""
    f32 = torch.float32
    qs, ks, vs = ac._sites(q, B, fq, hw, heads, f32), ac._sites(k, B, fk, hw, heads, f32), ac._sites(v, B, fk, hw, heads, f32)
    s = (qs @ ks.transpose(-1, -2)) * scale
    e = torch.exp(s - s.max(-1, keepdim=True).values)
    return ac._rows((e * (1.0 / e.sum(-1, keepdim=True))) @ vs).to(H).contiguous()


def temporal_restated(q, k, v, B, fq, fk, hw, heads, scale):
    """the dispatch of ops.temporal_attention and vsx_temporal_attention_f16"""
    d = q.shape[-1] // heads

    def one(q, k, v, B, fq):
        if d in (40, 80, 160) and fq <= 32 and fk <= 32:
            return temporal_packed(q, k, v, B, fq, fk, hw, heads, scale)
        if d in (40, 80, 160) and fq <= 32 and fk <= 128:
            return temporal_long(q, k, v, B, fq, fk, hw, heads, scale)
        return temporal_valu(q, k, v, B, fq, fk, hw, heads, scale)
    if fq <= 32 or fk > 128:
        return one(q, k, v, B, fq)
    out = torch.empty(q.shape[0], q.shape[1], dtype=H)                 # blocks of 32 query frames, one launch per (b, block)
    for b in range(B):
        kb, vb = k[b * fk * hw:(b + 1) * fk * hw], v[b * fk * hw:(b + 1) * fk * hw]
        for f0 in range(0, fq, 32):
            n = min(32, fq - f0)
            r0 = (b * fq + f0) * hw
            out[r0:r0 + n * hw] = one(q[r0:r0 + n * hw], kb, vb, 1, n)
    return out


class Tiled:
    """the restatements in the kernels' place"""
    set_option = staticmethod(lambda name, value: None)
    attention = staticmethod(lambda *a, **kw: flash_tiled(*a, **kw)[0])
    attention_lse = staticmethod(flash_tiled)
    attention_bwd = staticmethod(bwd_tiled)
    temporal_attention = staticmethod(temporal_restated)


IMPLS = {'standin': host_emulation, 'ideal': Ideal, 'tiled': Tiled}


def run_all(cases, runner, ident):
    """every case; one failure does not hide the others"""
    bad = []
    for c in cases:
        try:
            runner(c)
        except AssertionError as e:
            bad.append((ident(c), e.args[0][1] if e.args and isinstance(e.args[0], tuple) and len(e.args[0]) > 1 else str(e)))
    assert not bad, bad


# ---- 1. stand-ins, ideals and restatements stay inside every bound ----
@pytest.mark.parametrize('impl', IMPLS)
@pytest.mark.parametrize('table', ac.FLASH_TABLES)
def test_flash_forward(table, impl):
    run_all(ac.FLASH_TABLES[table], lambda c: ac.run_flash(IMPLS[impl], CPU, c), ac.flash_id)


@pytest.mark.parametrize('impl', IMPLS)
@pytest.mark.parametrize('cases', [ac.BWD_CASES, ac.BWD_CHAINED], ids=['alone', 'chained'])
def test_flash_backward(cases, impl):
    run_all(cases, lambda c: ac.run_bwd(IMPLS[impl], CPU, c), ac.bwd_id)


@pytest.mark.parametrize('impl', IMPLS)
@pytest.mark.parametrize('table', ac.TEMPORAL_TABLES)
def test_temporal(table, impl):
    run_all(ac.TEMPORAL_TABLES[table], lambda c: ac.run_temporal(IMPLS[impl], CPU, c), ac.temporal_id)


def test_materialised_path_standin():
    """its ideal IS the stand-in chain: what this proves is the per-element bound against fp64"""
    run_all(ac.MAT_CASES, lambda c: ac.run_materialised(host_emulation, CPU, c), ac.mat_id)


def test_materialised_backward_standin():
    from videoswap_amd import autograd as vsx_autograd

    def backward(*a):
        with host_emulation.installed(), torch.no_grad():
            return vsx_autograd._attention_backward(*a)
    run_all(ac.MAT_BWD_CASES, lambda c: ac.run_materialised_bwd(backward, CPU, c), ac.mat_id)


def test_at_most_five_percent_of_the_cases_are_left_out():
    total = (sum(len(t) for t in ac.FLASH_TABLES.values()) + len(ac.BWD_CASES) + len(ac.BWD_CHAINED)
             + sum(len(t) for t in ac.TEMPORAL_TABLES.values()) + len(ac.MAT_CASES) + len(ac.MAT_BWD_CASES))
    assert len(LEFT_OUT) <= 0.05 * total, (len(LEFT_OUT), total)


def test_lse_bound_is_the_derived_one():
    want = torch.tensor([[[0.5, -40.0, 3000.0]]], dtype=torch.float64)
    ok = want + torch.tensor([7.0e-4, -7.0e-4 - 39e-6, 7.0e-4 + 2.4e-3])       # 1.4427 2^-11 = 7.04e-4; 2^-20 |want|
    lse = torch.zeros(1, 1, 64)
    lse[..., :3] = ok.float()
    ac.check_lse('lse bound', lse, want, want.float(), 3)
    del ac.FIGURES[-1]


# ---- 2. mutants ----
def _rejected(what, runner):
    before = len(ac.FIGURES)
    with pytest.raises(AssertionError) as e:
        runner()
    del ac.FIGURES[before:]                                           # a mutant's figures are no parity figures
    name, failed = e.value.args[0][0], e.value.args[0][1]
    assert failed and isinstance(failed, list), e.value                # rejected by the RULE, not by some other assertion
    print(f'mutant {what}: rejected by {failed} ({name})')


DOMLAST = dict(heads=3, fn='attention_lse', kind='domlast')
FWD_MUTANTS = [
    ('drop_last', ac._fc(129, 65)),                                   # key nk - 1 dropped
    ('count_pad', ac._fc(129, 65)),                                   # one zero-padded key counted
    ('count_pad', ac._fc(33, 65, d=64, heads=2, kind='q0v1')),        # ... which the exact 1.0 of softmax(0) @ 1 alone shows
    ('no_o_rescale', ac._fc(33, 65, d=40, **DOMLAST)),                # O not rescaled when the max grows in the last tile
    ('no_l_rescale', ac._fc(33, 65, d=64, **DOMLAST)),                # l not rescaled while O is
    ('q128_from_q0', ac._fc(129, 65)),                                # query 128 computed from query 0
    ('wide_qk', ac._fc(65, 65, d=40, view='halves')),                 # the QK product over 48 channels of a 2C-wide view
    ('lse_off', ac._fc(129, 65, fn='attention_lse')),                 # lse off by 2e-3
    ('lse_nomax', ac._fc(129, 65, fn='attention_lse')),               # lse without its max term
]


@pytest.mark.parametrize('mutant,case', FWD_MUTANTS, ids=[f'{m}-{ac.flash_id(c)}' for m, c in FWD_MUTANTS])
def test_flash_forward_mutant_is_rejected(mutant, case):
    assert any(case == c for t in ac.FLASH_TABLES.values() for c in t), 'a mutant must be caught by a case OF THE TABLES'

    def fn(*a, **kw):
        res = flash_tiled(*a, mutant=mutant, **kw)
        return res if case['fn'] == 'attention_lse' else res[0]
    _rejected(mutant, lambda: ac.run_flash(Tiled, CPU, case, fn=fn))


BWD_MUTANTS = [('delta_half', ac._bc(65, 129)),                       # delta from half the channels
               ('no_scale', ac._bc(65, 129)),                         # dS without scale
               ('drop_q64', ac._bc(65, 129)),                         # the contributions of query 64 to dk / dv dropped
               ('drop_q64', ac._bc(65, 129, d=80))]


@pytest.mark.parametrize('mutant,case', BWD_MUTANTS, ids=[f'{m}-{ac.bwd_id(c)}' for m, c in BWD_MUTANTS])
def test_flash_backward_mutant_is_rejected(mutant, case):
    assert case in ac.BWD_CASES
    _rejected(mutant, lambda: ac.run_bwd(Tiled, CPU, case, fn=lambda *a, **kw: bwd_tiled(*a, mutant=mutant, **kw)))


def test_an_unmasked_padding_key_cannot_move_dq():
    """Key 65's zero padding left unmasked in the dQ kernel at nk = 65 is an EQUIVALENT mutant, so no rule can reject it: its
    dS is not zero (P = exp2(-lse), dP = 0, delta != 0), but dQ^T += K^T dS^T multiplies it with the zero column that
    ops.attention_bwd pads K^T with (and the descriptor's zero fill beyond).  Bit-identical to the unmutated restatement."""
    case = ac._bc(129, 65)
    q, k, v, dout = ac.bwd_inputs(case, CPU)
    out, lse = flash_tiled(q, k, ac.make_vt(v), 2, 40 ** -0.5)
    a = bwd_tiled(q, k, v, out, dout, lse, 2, 40 ** -0.5)
    b = bwd_tiled(q, k, v, out, dout, lse, 2, 40 ** -0.5, mutant='dq_pad_unmasked')
    assert all(torch.equal(x, y) for x, y in zip(a, b))


T_MUTANTS = [('offdiag', ac._tc(16, 16, 40, heads=8)),                # the off-diagonal head blocks not masked
             ('padkeys', ac._tc(16, 5, 40, heads=8)),                 # padding keys not masked
             ('padkeys', ac._tc(16, 5, 160, heads=5, hw=1, B=2, out=1))]


@pytest.mark.parametrize('mutant,case', T_MUTANTS, ids=[f'{m}-{ac.temporal_id(c)}' for m, c in T_MUTANTS])
def test_temporal_mutant_is_rejected(mutant, case):
    ac.run_temporal(Tiled, CPU, case)                                 # unmutated, the same restatement passes
    del ac.FIGURES[-1]
    _rejected(mutant, lambda: ac.run_temporal(Tiled, CPU, case, fn=lambda *a: temporal_packed(*a, mutant=mutant)))
