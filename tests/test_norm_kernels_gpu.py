"""GPU parity tests of the forward normalisation kernels (videoswap_amd/csrc/norm.hip: GroupNorm statistics / finalize / apply,
LayerNorm, the row statistics of the folded LayerNorm and their combine) and of the scalar glue of csrc/elementwise.hip, each on
its own against an fp64 reference: at the indexing edges of every kernel, and up a ladder of inputs whose mean dwarfs their spread.

Cases, references and the rule live in tests/norm_case.py (shared with the CPU proof of the rule, tests/test_norm_case.py).  The
two-pass kernels are held to the fp32 two-pass ideal on every rung; the one-pass kernels to a float32 restatement of their own form,
widened by the measured spread between summation orders and by nothing else.  Every call goes through videoswap_amd.ops; `_lib`
only where ops has no wrapper (vsx_groupnorm_stats alone, vsx_row_stats_combine on given parts, refusals that must leave a
buffer untouched).  Figures and the measured envelope per kernel: profiles/norm_kernel_parity.json (VSX_WRITE_PROFILES=1).
"""
import json
import os

import pytest
import torch

import norm_case as nc
from util import ROOT

pytestmark = pytest.mark.gpu
DEV = 'cuda'
H = torch.float16


def ops():
    from videoswap_amd import ops as _ops
    return _ops


def lib():
    from videoswap_amd import _lib
    return _lib


# ---- GroupNorm ----
@pytest.mark.parametrize('run', nc.gn_runs(), ids=nc.gn_id)
def test_group_norm(run):
    nc.run_group_norm(ops(), DEV, run)


def test_group_norm_chunk_counts():
    """the table aims at 64 | 65 chunks (the fused finalize's limit), 263 (the finalize kernel's strided loop) and the 1024-row
    cap: a change of gn_stat_rows must show up here, as cases to re-aim, not as a silent loss of the edges"""
    count = lib().load().vsx_groupnorm_chunks
    for (nimg, rows), n in nc.GN_CHUNKS.items():
        assert count(rows, nimg) == n, (nimg, rows)
    for c in nc.GN_CASES:
        assert count(c[1], c[0]) == nc.gn_chunks(c[1], c[0]), c


def gpu_partials(xb, nimg, groups):
    o, L = ops(), lib()
    C = xb.shape[-1]
    rows = xb.numel() // C // nimg
    nch = L.load().vsx_groupnorm_chunks(rows, nimg)
    partial = torch.empty(nimg, nch, groups, 2, dtype=torch.float32, device=xb.device)
    L.check(L.load().vsx_groupnorm_stats(o._p(xb), None, nimg, rows, C, 0, groups, o._p(partial), o._stream()), 'vsx_groupnorm_stats')
    return partial


@pytest.mark.parametrize('rung', nc.GATHER_RUNGS, ids=lambda r: nc.LADDER[r][0])
def test_group_norm_from_gathered_partials(rung):
    nc.run_group_norm_gathered(ops(), DEV, rung, gpu_partials)


# ---- LayerNorm, row statistics ----
@pytest.mark.parametrize('run', nc.LN_RUNS, ids=nc.ln_id)
def test_layer_norm(run):
    nc.run_layer_norm(ops(), DEV, run)


def test_layer_norm_refusals_leave_the_output_untouched():
    o, L = ops(), lib()
    fn = L.load().vsx_layernorm
    flat = torch.ones(4 * 64 + 8, dtype=H, device=DEV)
    for what, x, M, C in (('C % 8', flat, 4, 12), ('C > 2048', torch.ones(2, 2056, dtype=H, device=DEV), 2, 2056),
                          ('misaligned', flat[1:1 + 4 * 64], 4, 64)):
        gamma, beta = torch.ones(C, dtype=H, device=DEV), torch.zeros(C, dtype=H, device=DEV)
        y = torch.full((M * C,), 7.0, dtype=H, device=DEV)
        rc = fn(o._p(x), M, C, o._p(gamma), o._p(beta), 1e-5, None, 0, 0, 0, o._p(y), o._stream())
        torch.cuda.synchronize()
        assert rc != 0, what
        assert bool((y == 7.0).all()), what
    with pytest.raises(L.VsxError):
        o.layer_norm(flat[:48].view(4, 12), torch.ones(12, dtype=H, device=DEV), torch.zeros(12, dtype=H, device=DEV))
    with pytest.raises(L.VsxError):
        o.layer_norm(flat[1:1 + 4 * 64].view(4, 64), torch.ones(64, dtype=H, device=DEV), torch.zeros(64, dtype=H, device=DEV))
    y = o.layer_norm(flat[:4 * 64].view(4, 64), torch.ones(64, dtype=H, device=DEV), torch.zeros(64, dtype=H, device=DEV))
    assert y.shape == (4, 64)                                                   # the same call with a legal shape goes through


def row_stats(x, eps):
    o = ops()
    ln = o.DeferredLN(x, torch.ones(x.shape[-1], dtype=H, device=x.device), torch.zeros(x.shape[-1], dtype=H, device=x.device), eps)
    assert ln.row_parts is None                                                 # a pass over x: vsx_row_stats
    return ln.stats()


@pytest.mark.parametrize('run', nc.RS_RUNS, ids=nc.rs_id)
def test_row_stats(run):
    nc.run_row_stats(row_stats, DEV, run)


def combine(parts, C, eps):
    o, L = ops(), lib()
    M = parts.shape[0]
    st = torch.full((M, 2), float('nan'), dtype=torch.float32, device=parts.device)
    L.check(L.load().vsx_row_stats_combine(o._p(parts), M, parts.shape[1], C, float(eps), o._p(st), o._stream()), 'vsx_row_stats_combine')
    return st


@pytest.mark.parametrize('run', nc.COMBINE_RUNS, ids=nc.combine_id)
def test_row_stats_combine(run):
    nc.run_row_stats_combine(combine, DEV, run)


def test_row_stats_combine_refuses_65_parts():
    parts = torch.ones(4, 65, 2, dtype=torch.float32, device=DEV)
    with pytest.raises(lib().VsxError):
        combine(parts, 320, 1e-5)
    assert torch.isfinite(combine(parts[:, :64].contiguous(), 320, 1e-5)).all()


# ---- LayerNorm folded into the consuming Linear ----
def folded(x, gamma, beta, eps, pe, rpf, frames, off, w, b, residual, geglu):
    o = ops()
    return o.linear(o.DeferredLN(x, gamma, beta, eps, pe, rpf, frames, off), w, b, residual=residual, geglu=geglu)


@pytest.mark.parametrize('run', nc.FOLD_RUNS, ids=nc.fold_id)
def test_layer_norm_folded_into_linear(run):
    nc.run_folded(folded, DEV, run)


# ---- the scalar glue of csrc/elementwise.hip ----
@pytest.mark.parametrize('guidance', nc.DDIM_GUIDANCE, ids=lambda g: f'guidance{g}')
@pytest.mark.parametrize('alphas', nc.DDIM_ALPHAS, ids=lambda a: f'alpha{a[0]}-{a[1]}')
@pytest.mark.parametrize('n', nc.EW_SIZES)
def test_cfg_ddim_step(n, alphas, guidance):
    nc.run_cfg_ddim(ops(), DEV, n, alphas, guidance)


def test_cfg_ddim_step_refuses_alphas_outside_0_1():
    x = torch.zeros(16, dtype=H, device=DEV)
    for a_t, a_n in nc.DDIM_REFUSED:
        with pytest.raises(lib().VsxError):
            ops().cfg_ddim_step(x, x, x, 7.5, a_t, a_n)
    assert ops().cfg_ddim_step(x, x, x, 7.5, 1.0, 1.0).shape == x.shape


@pytest.mark.parametrize('n', nc.EW_SIZES)
def test_masked_blend(n):
    nc.run_masked_blend(ops(), DEV, n)


@pytest.mark.parametrize('s', nc.AXPY_S)
@pytest.mark.parametrize('n', nc.EW_SIZES)
def test_axpy(n, s):
    nc.run_axpy(ops(), DEV, n, s)


@pytest.mark.parametrize('case', nc.PACK_CASES, ids=lambda c: 'x'.join(str(v) for v in c))
def test_pack_latents(case):
    nc.run_pack(ops(), DEV, case)


@pytest.mark.parametrize('case', nc.UNPACK_CASES, ids=lambda c: 'x'.join(str(v) for v in c))
def test_unpack_latents(case):
    nc.run_unpack(ops(), DEV, case)


def test_parity_figures_recorded():
    """runs after the parity cases (file order): all of them left their figures; VSX_WRITE_PROFILES=1 writes the profile.  The
    envelope — per kernel, the largest mean / std of the ladder up to which it meets the TWO-PASS rule — is recorded, not asserted"""
    assert len(nc.FIGURES) == nc.expected_figures()
    env = nc.envelopes()
    print(json.dumps(env, indent=1))
    if os.environ.get('VSX_WRITE_PROFILES') == '1':
        out = os.environ.get('VSX_PROFILE_DIR', os.path.join(ROOT, 'profiles'))
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, 'norm_kernel_parity.json'), 'w') as f:
            json.dump({'device': torch.cuda.get_device_name(0), 'rule': nc.RULE, 'spread': nc.SPREAD,
                       'ladder': [dict(rung=r[0], mean_over_std=r[4]) for r in nc.LADDER], 'envelope': env,
                       'cases': nc.FIGURES}, f, indent=1)
