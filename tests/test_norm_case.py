"""The cases and the rule of tests/norm_case.py, proven on the CPU before a GPU sees them.

1. Every case of the GPU table (tests/test_norm_kernels_gpu.py) except the 2^20-row one runs with the stand-ins of
   tests/host_emulation.py (or, where it has none, an fp32 statement of the contract below) in the kernel's place.
2. SPREAD, the only constant of the one-pass rule, is recomputed from the references and must not exceed what is written down.
3. A correct one-pass GroupNorm restated with the kernels' structure passes the form rule on every rung and FAILS the plain
   two-pass rule on the top rungs: the ladder bites, and the form rule is no blanket waiver — which the mutants prove again:
4. Deliberate mutants, the mistakes a normalisation kernel can make, are each REJECTED by the rule.
"""
import pytest
import torch
import torch.nn.functional as F

import host_emulation
import norm_case as nc

CPU = 'cpu'
GN_RUNS = nc.gn_runs(with_huge=False)


# ---- stand-ins where tests/host_emulation.py has none: the contract in fp32, other arithmetic than the references ----
def row_stats_standin(x, eps):
    var, mean = torch.var_mean(x.float(), dim=-1, unbiased=False)
    rstd = (var + eps).rsqrt()
    return torch.stack([rstd, -rstd * mean], dim=-1)


def combine_standin(parts, C, eps, nparts_max=64):
    assert parts.shape[1] <= nparts_max
    s, q = parts[..., 0].sum(1), parts[..., 1].sum(1)
    mean = s / C
    rstd = ((q / C - mean * mean).clamp_min(0) + eps).rsqrt()
    return torch.stack([rstd, -rstd * mean], dim=-1)


def folded_standin(x, gamma, beta, eps, pe, rpf, frames, off, w, b, residual, geglu):
    y = F.layer_norm(x.float(), (x.shape[-1],), gamma.float(), beta.float(), eps)
    if pe is not None:
        y = y + pe.float()[(torch.arange(x.shape[0]) // rpf) % frames + off]
    y = F.linear(y, w.float(), b.float())
    if geglu:
        h, g = y.chunk(2, dim=-1)
        y = h * F.gelu(g)
    return (y if residual is None else y + residual.float()).to(nc.H)


# ---- 1. the stand-ins stay inside every bound ----
@pytest.mark.parametrize('run', GN_RUNS, ids=nc.gn_id)
def test_group_norm_standin(run):
    nc.run_group_norm(host_emulation, CPU, run)


@pytest.mark.parametrize('rung', nc.GATHER_RUNGS)
def test_group_norm_gathered_standin(rung):
    nc.run_group_norm_gathered(host_emulation, CPU, rung, nc.host_partials)


def test_chunk_counts_of_the_table():
    for (nimg, rows), n in nc.GN_CHUNKS.items():
        assert nc.gn_chunks(rows, nimg) == n


@pytest.mark.parametrize('run', nc.LN_RUNS, ids=nc.ln_id)
def test_layer_norm_standin(run):
    nc.run_layer_norm(host_emulation, CPU, run)


@pytest.mark.parametrize('run', nc.RS_RUNS, ids=nc.rs_id)
def test_row_stats_standin(run):
    nc.run_row_stats(row_stats_standin, CPU, run)


@pytest.mark.parametrize('run', nc.COMBINE_RUNS, ids=nc.combine_id)
def test_row_stats_combine_standin(run):
    nc.run_row_stats_combine(combine_standin, CPU, run)


@pytest.mark.parametrize('run', nc.FOLD_RUNS, ids=nc.fold_id)
def test_folded_standin(run):
    nc.run_folded(folded_standin, CPU, run)


@pytest.mark.parametrize('n', nc.EW_SIZES)
def test_elementwise_standins(n):
    for alphas in nc.DDIM_ALPHAS:
        for guidance in nc.DDIM_GUIDANCE:
            nc.run_cfg_ddim(host_emulation, CPU, n, alphas, guidance)
    nc.run_masked_blend(host_emulation, CPU, n)
    for s in nc.AXPY_S:
        nc.run_axpy(host_emulation, CPU, n, s)


def test_pack_unpack_standins():
    for case in nc.PACK_CASES:
        nc.run_pack(host_emulation, CPU, case)
    for case in nc.UNPACK_CASES:
        nc.run_unpack(host_emulation, CPU, case)


def test_figures_of_a_full_pass():
    """runs after the stand-in cases (file order)"""
    assert len(nc.FIGURES) == nc.expected_figures(with_huge=False)
    env = nc.envelopes()
    assert set(env) == {'group_norm', 'group_norm_gathered', 'layer_norm', 'row_stats', 'row_stats_combine', 'folded_layer_norm plain',
                        'folded_layer_norm pe', 'folded_layer_norm geglu', 'folded_layer_norm residual'}
    for kernel in ('layer_norm', 'row_stats'):              # two-pass: the whole ladder
        assert all(env[kernel]['meets_two_pass_rule'].values()), env[kernel]


# ---- 2. SPREAD, and where the fold takes the form rule ----
SPREAD_HOST_TOL = 1.03          # the measured ratio moves in its third digit with the host's torch.sum / matmul order


@pytest.mark.parametrize('which', sorted(nc.SPREAD))
def test_spread_is_what_the_references_give(which):
    got, table = nc.measure_spread(which)
    print(which, got, table)
    for m, v in got.items():
        assert v <= SPREAD_HOST_TOL * nc.SPREAD[which][m], (which, m, v, nc.SPREAD[which][m])
        assert nc.SPREAD[which][m] <= 1.25 * v + 0.1, ('written down far above what the references give', which, m, v)


def fold_form_restatement(order):
    def fn(x, gamma, beta, eps, pe, rpf, frames, off, w, b, residual, geglu):
        return nc.form_ln_linear(x, gamma, beta, eps, w, b, pe, rpf, frames, off, residual, geglu, order=order)
    return fn


@pytest.mark.parametrize('run', nc.FOLD_RUNS, ids=nc.fold_id)
def test_fold_takes_the_form_rule_only_where_its_restatement_misses_the_two_pass_rule(run):
    """FOLD_FORM_RUNGS against the references alone: the float32 restatement of the fold's form is run as if it were the kernel.
    Outside the table it must meet the unchanged two-pass rule (the rule asserted there); inside the table it must be AT or beyond a
    two-pass bound (>= 0.95 of it in some metric: the table names departures of the form, not rungs that are merely convenient)"""
    kind, rung = run[3], run[4]
    before = len(nc.FIGURES)
    try:
        fig = nc.run_folded(fold_form_restatement('chunk64'), CPU, run)
    finally:
        del nc.FIGURES[before:]
    if rung in nc.FOLD_FORM_RUNGS[kind]:
        assert max(fig[m + '_form_two_pass_ratio'] for m in nc.METRICS) >= 0.95, fig
    else:
        assert fig['asserted'] == 'two_pass' and fig['two_pass_rule'], fig


# ---- 3. a correct one-pass GroupNorm with the kernels' structure, and its mutants ----
def gn_one_pass(x, gamma, beta, groups, eps, nimg, silu=False, x2=None, partial_hook=None, count_rows=None, mutant=None):
    """vsx_groupnorm_stats / _apply restated in fp32: per-chunk (sum, sum of squares) of every group, chunks added in index order,
    var = q / n - mean^2, per-channel a = rstd gamma, b = beta - mean a, y = x a + b.  `mutant` breaks one step."""
    xin = (x if x2 is None else torch.cat([x, x2], dim=-1)).float()
    _, rows, C = xin.shape
    cpg = C // groups
    ch = torch.arange(C)
    lookup = (ch // 8 * 8) // cpg if mutant == 'straddle' else ch // cpg      # mutant: a vector's FIRST channel decides its group
    stat_in = xin.clone()
    if mutant == 'skip_last_row':
        stat_in[:, rows - 1] = 0.0                                            # the last (ragged) row never enters a partial sum
    if mutant == 'no_x2' and x2 is not None:
        stat_in[..., x.shape[-1]:] = 0.0                                      # the second source never enters a partial sum
    rpc = min(max(rows * nimg // 768, 8), 1024)
    nch = (rows + rpc - 1) // rpc
    t = F.pad(stat_in, (0, 0, 0, nch * rpc - rows)).view(nimg, nch, rpc, groups, cpg)
    if mutant == 'fp16_stats':                                                # every addition rounded to fp16
        t = t.reshape(nimg, nch * rpc, groups * cpg)
        s, q = torch.zeros(nimg, C), torch.zeros(nimg, C)
        for r in range(t.shape[1]):
            s, q = (s + t[:, r]).to(nc.H).float(), (q + t[:, r] * t[:, r]).to(nc.H).float()
        partial = torch.stack([s.view(nimg, groups, cpg).sum(-1), q.view(nimg, groups, cpg).sum(-1)], dim=-1).to(nc.H).float()[:, None]
    else:
        partial = torch.stack([t.sum((2, 4)), (t * t).sum((2, 4))], dim=-1)     # [nimg, nch, groups, 2]
    if partial_hook is not None:
        partial = partial_hook(partial.contiguous())
    tot = torch.zeros(nimg, groups, 2)
    for c in range(partial.shape[1]):
        tot = tot + partial[:, c]
    n = float((rows if count_rows is None or mutant == 'count_rows' else count_rows) * cpg)
    mean = tot[..., 0] / n
    var = (tot[..., 1] / n - mean * mean).clamp_min(0)
    if mutant == 'n_minus_1':
        var = var * (n / (n - 1.0))
    rstd = 1.0 / (var.sqrt() + eps) if mutant == 'eps_outside' else (var + eps).rsqrt()
    ga, be = gamma.float(), beta.float()
    if mutant == 'silu_first':
        xh = (xin - mean[:, None, lookup]) * rstd[:, None, lookup]
        return (xh * torch.sigmoid(xh) * ga + be).to(nc.H)
    a = rstd[:, None, lookup] * ga
    y = xin * a + (be - mean[:, None, lookup] * a)
    return (y * torch.sigmoid(y) if silu else y).to(nc.H)


def _ladder_run(rung):
    return nc.GN_LADDER + (rung, False, nc.EPS, False)


@pytest.mark.parametrize('run', [r for r in GN_RUNS if r[1] <= 2100], ids=nc.gn_id)
def test_one_pass_restatement_passes_the_form_rule(run):
    before = len(nc.FIGURES)
    nc.run_group_norm(host_emulation, CPU, run, fn=gn_one_pass)       # (host_emulation: its silu for the group of zeros)
    del nc.FIGURES[before:]


def _rejected(what, runner):
    before = len(nc.FIGURES)
    with pytest.raises(AssertionError) as e:
        runner()
    del nc.FIGURES[before:]                                           # a mutant's figures are no parity figures
    name, failed = e.value.args[0][0], e.value.args[0][1]
    assert failed and isinstance(failed, list), e.value                # rejected by the RULE, not by some other assertion
    print(f'{what}: rejected by {failed} ({name})')


@pytest.mark.parametrize('rung', [4, 5], ids=lambda r: nc.LADDER[r][0])
def test_one_pass_restatement_fails_the_two_pass_rule_on_the_top_rungs(rung):
    """uniform * 0.5 + 16 and + 32: correct one-pass arithmetic is outside what a two-pass kernel is held to"""
    _rejected('one-pass under the two-pass rule', lambda: nc.run_group_norm(None, CPU, _ladder_run(rung), fn=gn_one_pass, rule='two_pass'))


RAGGED = (3, 50, 64, 0, 32, 0, False, nc.EPS, False)
FEW = (1, 5, 8, 0, 1, 0, True, nc.EPS, False)
CPG1 = (2, 33, 64, 0, 64, 0, False, nc.EPS, False)
CONCAT = (2, 77, 640, 320, 32, 0, True, nc.EPS, False)
TINY = nc.GN_ZERO + ('tiny', False, nc.EPS, False)
GN_MUTANTS = [('n_minus_1', _ladder_run(0)), ('n_minus_1', FEW), ('eps_outside', TINY), ('straddle', _ladder_run(0)), ('straddle', CPG1),
              ('skip_last_row', RAGGED), ('skip_last_row', FEW), ('no_x2', CONCAT), ('fp16_stats', _ladder_run(0)),
              ('fp16_stats', _ladder_run(1)), ('silu_first', CONCAT), ('silu_first', FEW)]


@pytest.mark.parametrize('mutant,run', GN_MUTANTS, ids=[f'{m}-{nc.gn_id(r)}' for m, r in GN_MUTANTS])
def test_group_norm_mutant_is_rejected(mutant, run):
    def fn(*a, **k):
        return gn_one_pass(*a, mutant=mutant, **k)
    _rejected(mutant, lambda: nc.run_group_norm(None, CPU, run, fn=fn))


@pytest.mark.parametrize('rung', nc.GATHER_RUNGS)
def test_gathered_mutant_count_rows_ignored_is_rejected(rung):
    def fn(*a, **k):
        return gn_one_pass(*a, mutant='count_rows', **k)
    before = len(nc.FIGURES)
    nc.run_group_norm_gathered(None, CPU, rung, nc.host_partials, fn=gn_one_pass)        # unmutated: passes
    del nc.FIGURES[before:]
    _rejected('count_rows ignored', lambda: nc.run_group_norm_gathered(None, CPU, rung, nc.host_partials, fn=fn))


def ln_mutant(mutant):
    def fn(x, gamma, beta, eps, pe=None, rows_per_frame=0, frames=0, frame_offset=0):
        xf = x.float()
        C = x.shape[-1]
        mean = xf.mean(-1, keepdim=True)
        var = ((xf - mean) ** 2).sum(-1, keepdim=True) / (C - 1 if mutant == 'n_minus_1' else C)
        rstd = 1.0 / (var.sqrt() + eps) if mutant == 'eps_outside' else (var + eps).rsqrt()
        y = (xf - mean) * rstd * gamma.float() + beta.float()
        if pe is not None:
            idx = torch.arange(x.shape[0]) // rows_per_frame
            if mutant != 'no_modulo':
                idx = idx % frames
            if mutant != 'no_frame_offset':
                idx = idx + frame_offset
            y = y + pe.float()[idx.clamp_max(pe.shape[0] - 1)]
        return y.to(nc.H)
    return fn


LN_MUTANTS = [('no_frame_offset', (48, 320, 6, 4, 2, 0)), ('no_frame_offset', (10, 1280, 5, 1, 3, 0)), ('no_modulo', (48, 320, 6, 4, 2, 0)),
              ('no_modulo', (24, 64, 1, 24, 0, 0)), ('no_modulo', (10, 1280, 5, 1, 3, 0)), ('n_minus_1', (17, 320, 0, 0, 0, 0)),
              ('eps_outside', (17, 320, 0, 0, 0, 'tiny'))]


@pytest.mark.parametrize('run', [r for r in nc.LN_RUNS if r[0] <= 48], ids=nc.ln_id)
def test_layer_norm_restatement_passes_unmutated(run):
    before = len(nc.FIGURES)
    nc.run_layer_norm(None, CPU, run, fn=ln_mutant(None))
    del nc.FIGURES[before:]


@pytest.mark.parametrize('mutant,run', LN_MUTANTS, ids=[f'{m}-{nc.ln_id(r)}' for m, r in LN_MUTANTS])
def test_layer_norm_mutant_is_rejected(mutant, run):
    if mutant == 'no_modulo' and run[:2] == (24, 64):
        # 24 frames of one row each, all inside the table: without the modulo nothing changes, and the rule must NOT object
        before = len(nc.FIGURES)
        nc.run_layer_norm(None, CPU, run, fn=ln_mutant(mutant))
        del nc.FIGURES[before:]
        return
    _rejected(mutant, lambda: nc.run_layer_norm(None, CPU, run, fn=ln_mutant(mutant)))


def test_statistics_mutants_are_rejected():
    """the fp32 statistics rule: variance over n - 1, and a combine that drops its last part"""
    def rs(x, eps):
        var, mean = torch.var_mean(x.float(), dim=-1, unbiased=True)
        rstd = (var + eps).rsqrt()
        return torch.stack([rstd, -rstd * mean], dim=-1)
    _rejected('row_stats over n - 1', lambda: nc.run_row_stats(rs, CPU, (33, 1280, 0)))
    _rejected('combine without its last part',
              lambda: nc.run_row_stats_combine(lambda p, C, eps: combine_standin(p[:, :-1], C, eps), CPU, (33, 1280, '64', 0)))
    _rejected('combine under the two-pass bound alone', lambda: _combine_two_pass_only())


def _combine_two_pass_only():
    """a correct one-pass combine on the top rung, held to the two-pass restatement alone: the ladder bites here too"""
    x = nc.ln_inputs(*nc.COMBINE_LADDER, 5, CPU)[0]
    got = combine_standin(nc.combine_parts(x, 'gemm'), x.shape[-1], nc.EPS)
    nc.check_stats('combine two-pass only', got, nc.ref_row_stats(x, nc.EPS, torch.float64), nc.ref_row_stats(x, nc.EPS, torch.float32))
