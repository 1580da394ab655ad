"""GPU parity tests of the attention kernels (videoswap_amd/csrc/attention.hip: flash forward with and without lse, the three
temporal kernels; csrc/attention_bwd.hip: delta, dQ, dK / dV; the materialised scores -> softmax -> PV path and the backward
built on it), each on its own against an fp64 reference, at the smallest shapes at which a tile, mask or rescale can go wrong.

Cases, references, ideals and the comparison rule live in tests/attention_case.py (shared with the CPU proof of the rule,
tests/test_attention_case.py).  Every bound is taken from the contract ideal on the same inputs or derived from the fp16
roundings the contract names; nothing is tuned to what the kernels give.  Every call goes through videoswap_amd.ops.
Figures: profiles/attention_parity.json (VSX_WRITE_PROFILES=1).
"""
import json
import os

import pytest
import torch

import attention_case as ac
from util import ROOT

pytestmark = pytest.mark.gpu
DEV = 'cuda'
H = torch.float16


def ops():
    from videoswap_amd import ops as _ops
    return _ops


def vsx_error():
    from videoswap_amd._lib import VsxError
    return VsxError


@pytest.fixture(autouse=True)
def _figures_carry_their_test(request):
    n = len(ac.FIGURES)
    yield
    for fig in ac.FIGURES[n:]:
        fig['group'] = request.node.name


def run_all(cases, runner, ident):
    """every case of a group; one failure does not hide the others"""
    bad = []
    for c in cases:
        try:
            runner(c)
        except AssertionError as e:
            bad.append((ident(c), e.args[0][1:] if e.args and isinstance(e.args[0], tuple) else str(e)))
    assert not bad, bad


def by(cases, key):
    groups = {}
    for c in cases:
        groups.setdefault(key(c), []).append(c)
    return groups


# ---- flash forward ----
EDGES = by(ac.FLASH_EDGES, lambda c: c['nq'])


@pytest.mark.parametrize('nq', EDGES)
def test_flash_forward_tile_edges(nq):
    run_all(EDGES[nq], lambda c: ac.run_flash(ops(), DEV, c), ac.flash_id)


DIMS = by(ac.FLASH_DIMS, lambda c: c['d'])


@pytest.mark.parametrize('d', DIMS)
def test_flash_forward_head_dims_with_a_dominant_key(d):
    run_all(DIMS[d], lambda c: ac.run_flash(ops(), DEV, c), ac.flash_id)


VARIANTS = by(ac.FLASH_VARIANTS, lambda c: '-'.join(f'{k}{v}' for k, v in c['opts'].items()) or 'launch_rule')


@pytest.mark.parametrize('variant', VARIANTS)
def test_flash_forward_launch_variants(variant):
    run_all(VARIANTS[variant], lambda c: ac.run_flash(ops(), DEV, c), ac.flash_id)
    assert ops().get_option('attn_qb') == 0 and ops().get_option('attn_o16') == 0


@pytest.mark.parametrize('table', ['views', 'known', 'ranges'])
def test_flash_forward_views_known_answers_ranges(table):
    run_all(ac.FLASH_TABLES[table], lambda c: ac.run_flash(ops(), DEV, c), ac.flash_id)


def _raw_forward(lse, scale, out, q, k, vt, nb, heads, n, d):
    from videoswap_amd import _lib
    C = heads * d
    lib, p = _lib.load(), (lambda t: t.data_ptr())
    stream = torch.cuda.current_stream().cuda_stream
    if lse is None:
        return lib.vsx_attention_f16(p(q), p(k), p(vt), p(out), nb, heads, n, n, d, C, C, vt.shape[2], C, n * C, n * C,
                                     C * vt.shape[2], n * C, 1, scale, stream)
    return ops()._train_fn('vsx_attention_lse_f16')(p(q), p(k), p(vt), p(out), p(lse), lse.shape[-1], nb, heads, n, n, d, C, C,
                                                    vt.shape[2], C, n * C, n * C, C * vt.shape[2], n * C, 1, scale, stream)


@pytest.mark.parametrize('scale', [0.0, -0.158, float('nan'), float('inf')])
def test_flash_entry_points_refuse_a_scale_that_is_not_positive(scale):
    """the kernel takes the row max before scaling: scale <= 0 (or no number) is refused, and NOTHING is launched - the output,
    lse, delta and gradient buffers, allocated here and handed to the library directly, keep their sentinel"""
    nb, heads, n, d = 1, 2, 72, 40
    C = heads * d
    g = torch.Generator().manual_seed(5)
    q, k, v, dout = (torch.randn(nb, n, C, generator=g).to(H).to(DEV) for _ in range(4))
    vt = ac.make_vt(v)
    for name in ('attention', 'attention_lse'):
        with pytest.raises(vsx_error()):
            getattr(ops(), name)(q, k, vt, heads, scale)
    good_out, good_lse = ops().attention_lse(q, k, vt, heads, d ** -0.5)
    with pytest.raises(vsx_error()):
        ops().attention_bwd(q, k, v, good_out, dout, good_lse, heads, scale)
    out = torch.full((nb, n, C), 7.0, dtype=H, device=DEV)
    lse = torch.full((nb, heads, 128), 7.0, dtype=torch.float32, device=DEV)
    assert _raw_forward(None, scale, out, q, k, vt, nb, heads, n, d) != 0
    assert _raw_forward(lse, scale, out, q, k, vt, nb, heads, n, d) != 0
    dq, dk, dv = (torch.full((nb, n, C), 7.0, dtype=H, device=DEV) for _ in range(3))
    delta = torch.full((nb, heads, 128), 7.0, dtype=torch.float32, device=DEV)
    qt, kt, dot = (t.transpose(1, 2).contiguous() for t in (q, k, dout))
    p = (lambda t: t.data_ptr())
    rc = ops()._train_fn('vsx_attention_bwd_f16')(p(q), p(k), p(v), p(good_out), p(dout), p(qt), p(kt), p(dot), p(good_lse), p(delta),
                                                  p(dq), p(dk), p(dv), nb, heads, n, n, d, n, n, 128, 1, scale,
                                                  torch.cuda.current_stream().cuda_stream)
    assert rc != 0
    torch.cuda.synchronize()
    for t in (out, lse, delta, dq, dk, dv):
        assert bool((t == 7.0).all()), 'a kernel ran'
    # the same raw calls with a legal scale go through: it is the scale that was refused
    assert _raw_forward(lse, d ** -0.5, out, q, k, vt, nb, heads, n, d) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, good_out)


# ---- flash backward ----
BWD = by(ac.BWD_CASES, lambda c: f"d{c['d']}-nq{c['nq']}" if c['d'] == 40 and c['kv_div'] == 1 else f"d{c['d']}")


@pytest.mark.parametrize('group', BWD)
def test_flash_backward(group):
    run_all(BWD[group], lambda c: ac.run_bwd(ops(), DEV, c), ac.bwd_id)


@pytest.mark.parametrize('case', ac.BWD_CHAINED, ids=ac.bwd_id)
def test_flash_backward_chained_to_the_kernels_own_forward(case):
    ac.run_bwd(ops(), DEV, case)


def test_flash_backward_refusals():
    z = (lambda *s, dt=H: torch.zeros(*s, dtype=dt, device=DEV))

    def call(d=40, heads=2, nb=2, kv_div=1, need_kv=True, lds=128, nq=72, nk=72):
        C = heads * d
        return ops().attention_bwd(z(nb, nq, C), z(nb // kv_div, nk, C), z(nb // kv_div, nk, C), z(nb, nq, C), z(nb, nq, C),
                                   z(nb, heads, lds, dt=torch.float32), heads, d ** -0.5, kv_div=kv_div, need_kv=need_kv)
    assert not ops().attention_bwd_supported(160) and all(ops().attention_bwd_supported(d) for d in (40, 64, 80))
    for kw in (dict(d=160),                            # no flash backward for this head dim
               dict(kv_div=2, need_kv=True),           # key / value gradients of a shared context
               dict(lds=72), dict(lds=100)):           # statistics rows that are no multiple of 64
        with pytest.raises(vsx_error()):
            call(**kw)
    dq, dk, dv = call()                                # the same call with legal arguments goes through
    assert dq.shape == (2, 72, 80) and dk.shape == dv.shape == (2, 72, 80)
    dq, dk, dv = call(kv_div=2, need_kv=False)
    assert dk is None and dv is None


# ---- temporal ----
PACKED = by(ac.T_PACKED, lambda c: f"{c['fq']}x{c['fk']}-d{c['d']}")
LONG = by(ac.T_LONG, lambda c: f"fq{c['fq']}-d{c['d']}")


@pytest.mark.parametrize('group', PACKED)
def test_temporal_packed_heads(group):
    run_all(PACKED[group], lambda c: ac.run_temporal(ops(), DEV, c), ac.temporal_id)
    assert ops().get_option('temporal_out') == 0


@pytest.mark.parametrize('group', LONG)
def test_temporal_long_clip(group):
    run_all(LONG[group], lambda c: ac.run_temporal(ops(), DEV, c), ac.temporal_id)


def test_temporal_fallback_block_loop_views_and_scales():
    run_all(ac.T_OTHER, lambda c: ac.run_temporal(ops(), DEV, c), ac.temporal_id)


def test_temporal_refuses_what_does_not_fit_the_lds():
    c = ac.TEMPORAL_LDS_REFUSAL
    q, k, v = ac.temporal_inputs(c, DEV)
    with pytest.raises(vsx_error()):
        ops().temporal_attention(q, k, v, c['B'], c['fq'], c['fk'], c['hw'], c['heads'], c['d'] ** -0.5)


# ---- the materialised path ----
def test_materialised_scores_softmax_pv():
    run_all(ac.MAT_CASES, lambda c: ac.run_materialised(ops(), DEV, c), ac.mat_id)


@pytest.mark.parametrize('case', ac.MAT_BWD_CASES, ids=ac.mat_id)
def test_materialised_backward(case):
    from videoswap_amd import autograd as vsx_autograd
    ac.run_materialised_bwd(vsx_autograd._attention_backward, DEV, case)


def test_parity_figures_recorded():
    """runs after the parity cases (file order): all of them left their figures; VSX_WRITE_PROFILES=1 writes the profile: per
    test of this file, the worst figure of every metric beside the ideal's and as a fraction of its bound, with the case"""
    assert len(ac.FIGURES) == ac.expected_figures(), (len(ac.FIGURES), ac.expected_figures())
    if os.environ.get('VSX_WRITE_PROFILES') == '1':
        out = os.environ.get('VSX_PROFILE_DIR', os.path.join(ROOT, 'profiles'))
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, 'attention_parity.json'), 'w') as f:
            f.write('{"device": %s,\n "rule": %s,\n "tensors": %d,\n "groups": [\n'
                    % (json.dumps(torch.cuda.get_device_name(0)), json.dumps(ac.RULE), len(ac.FIGURES)))
            f.write(',\n'.join('  ' + json.dumps(g) for g in ac.summarise(ac.FIGURES)))
            f.write('\n ]}\n')
