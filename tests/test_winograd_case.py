"""The cases and the rule of the stage-by-stage Winograd parity (tests/winograd_case.py), proven on the CPU before a GPU sees them.

1. A restatement of vsx_conv3x3_winograd_f16 ON THE DESCRIPTOR runs in the kernels' place: it reads and writes the host memory the
   descriptor, U and the workspace point at (so a stray store lands in a guard band, as a kernel's would), has the three stages
   with their rounding points, honours every descriptor field the table uses, and leaves V and Mt in the workspace in the
   library's layout.  It is written with index arithmetic, thread by thread as the kernels count them (the references of
   winograd_case.py use padding, unfold and conv2d).  It passes every case of both classes under the same runner.
2. Inputs E meet their precondition (V, U, Mt fp16-exact in fp64) for the whole table: a table edit that breaks it fails here.
3. Every mutant of MUTANTS, planted in the restatement, is rejected by the case named next to it, which passes without it.
4. The refusals, through the restatement and through the library itself (it refuses before any launch, so this needs no GPU).
"""
import ctypes

import pytest
import torch

import gemm_case as gc
import test_gemm_case as tgc
import winograd_case as wc

CPU = 'cpu'
H = torch.float16
WG = 256                        # threads per workgroup of both transform kernels


def _mem(ptr, count, dtype=H):
    return tgc._mem(ptr, dtype, count)


def host_winograd(d, u_ptr, ws_ptr, mut=None):
    C1, C2, N, Hh, Ww, M = d.C1, d.C2, d.N, d.H, d.W, d.M
    C, tiles, nimg = C1 + C2, M // 4, M // (Hh * Ww)
    th, tw = Hh // 2, Ww // 2
    ws = _mem(ws_ptr, 16 * tiles * (C + N) + (N if mut == 'mt_one_tile_past_the_end' else 0))
    V = ws[:16 * tiles * C].view(16, tiles, C)
    t = torch.arange(tiles)

    # ---- input transform: thread gid = tile * (C / 8) + octet ----
    ith, itw = (tw, th) if mut == 'th_tw_swapped' else (th, tw)
    img, r = t // (th * tw), t % (th * tw)
    ti, tj = r // itw, r % itw
    org = 0 if mut == 'window_origin_2ti' else -1
    y = 2 * ti[:, None] + org + torch.arange(4)[None, :]
    x = 2 * tj[:, None] + org + torch.arange(4)[None, :]
    inside = ((y >= 0) & (y < Hh))[:, :, None] & ((x >= 0) & (x < Ww))[:, None, :]               # [tiles, 4 (rows), 4 (columns)]
    pix = (img[:, None, None] * Hh + y.clamp(0, Hh - 1)[:, :, None]) * Ww + x.clamp(0, Ww - 1)[:, None, :]
    if mut == 'padding_clamped_to_the_border':
        inside = torch.ones_like(inside)
    win = [_mem(d.A, nimg * Hh * Ww * C1).view(-1, C1)[pix]]
    if C2:
        x2 = _mem(d.A2, nimg * Hh * Ww * C2)
        cs = C1 if mut == 'x2_with_c1_stride' else C2
        win.append(x2[(pix[..., None] * cs + torch.arange(C2)) % x2.numel()])
    win = torch.cat(win, -1).float()                                                             # [tiles, 4, 4, C]
    win[~inside] = 0
    d0, d1, d2, d3 = win[:, 0], win[:, 1], win[:, 2], win[:, 3]                                  # down the columns: [tiles, 4 (columns), C]
    down = [d0 - d2, d1 + d2, d1 - d2 if mut == 'bt_row_sign' else d2 - d1, d1 - d3]
    if mut == 'v_rounded_after_the_column_pass':
        down = [s.half().float() for s in down]
    v = []
    for s in down:
        t0, t1, t2, t3 = s[:, 0], s[:, 1], s[:, 2], s[:, 3]
        v += [t0 - t2, t1 + t2, t2 - t1, t1 - t3]
    v = torch.stack(v, 0).half()                                                                 # [16 (4 a + b), tiles, C]
    if mut == 'xi_transposed_in_v':
        v = v.view(4, 4, tiles, C).transpose(0, 1).reshape(16, tiles, C)
    nthreads = tiles * (C // 8)
    ran = torch.ones(nthreads, dtype=torch.bool)
    if mut == 'input_last_partial_workgroup_dropped' and nthreads % WG:
        ran[nthreads // WG * WG:] = False
    ran = ran.view(tiles, C // 8).repeat_interleave(8, dim=1)                                     # [tiles, C]
    V[:, ran] = v[:, ran]

    # ---- the batched GEMM: fp32 sums of fp16 products, one rounding ----
    U = _mem(u_ptr, 16 * N * C).view(16, N, C)
    kk = C - C % 64 if mut == 'k_tail_dropped' and C > 64 else C
    mt = torch.bmm(V[:, :, :kk].float(), U[:, :, :kk].float().transpose(1, 2)).half()
    Mt = ws[16 * tiles * C:16 * tiles * (C + N)].view(16, tiles, N)
    Mt[:] = mt
    if mut == 'mt_one_tile_past_the_end':
        ws[16 * tiles * (C + N):] = mt[15, -1]

    # ---- output transform and epilogue: thread gid = tile * (N / 8) + octet ----
    ti, tj = r // tw, r % tw
    m = Mt.clone() if mut == 'output_summed_in_fp16' else Mt.float()
    m = m.view(4, 4, tiles, N)
    down = [(m[0] + m[1]) + m[2], (m[1] - m[2]) - m[3]]                                           # [b, tiles, N]
    yq = [a.float() for s in down for a in ((s[0] + s[1]) + s[2], (s[1] - s[2]) - s[3])]           # q = 2 p + pj
    bias = _mem(d.bias, N) if d.bias else None
    rpv = d.rows_per_vec if d.rowvec else 1
    rowvec = _mem(d.rowvec, ((M + rpv - 1) // rpv) * N).view(-1, N) if d.rowvec else None
    residual = _mem(d.residual, M * d.ldr) if d.residual else None
    nthreads = tiles * (N // 8)
    ran = torch.ones(nthreads, dtype=torch.bool)
    if mut == 'output_last_partial_workgroup_dropped' and nthreads % WG:
        ran[nthreads // WG * WG:] = False
    ran = ran.view(tiles, N // 8).repeat_interleave(8, dim=1)
    width = N + 8 if mut == 'store_n_plus_8_columns' and d.ldc > N else N
    Cm = _mem(d.C, (M - 1) * d.ldc + width)
    n = torch.arange(N)
    for q in range(4):
        pi, pj = (q & 1, q >> 1) if mut == 'q_halves_swapped' else (q >> 1, q & 1)
        row = (img * Hh + 2 * ti + pi) * Ww + 2 * tj + pj
        o = yq[q]
        if bias is not None and mut != 'bias_after_the_rounding':
            o = o + bias.float()[None, :]
        if rowvec is not None:
            vrow = (img * Hh + 2 * ti) * Ww + 2 * tj if mut == 'rowvec_once_per_tile' else row
            o = o + rowvec[vrow // rpv].float()
        if residual is not None:
            ldr = d.ldc if mut == 'residual_with_ldc' else d.ldr
            o = o + residual[(row[:, None] * ldr + n[None, :]) % residual.numel()].float()
        o = o.half()
        if bias is not None and mut == 'bias_after_the_rounding':
            o = o + bias[None, :]
        at = row[:, None] * d.ldc + n[None, :]
        Cm[at[ran]] = o[ran]
        if width > N:
            Cm[(row[:, None] * d.ldc + N + torch.arange(8)[None, :]).reshape(-1)] = 0


class HostImpl(wc.WinoQueries):
    """the restatement behind the interface the runners use; `mut` plants one mutant"""

    def __init__(self, mut=None):
        super().__init__()
        self.mut = mut
        from videoswap_amd import ops
        self.winograd_weights = ops.winograd_weights          # the product's own code: plain torch, runs where its weight lives

    def winograd(self, d, u_ptr, ws_ptr, ws_bytes):
        need = self.wino_workspace(d)
        if need == 0:
            return wc.VSX_E_UNSUPPORTED
        if ws_bytes < need:
            return wc.VSX_E_WORKSPACE
        host_winograd(d, u_ptr, ws_ptr, self.mut)
        return wc.VSX_OK

    def gemm(self, d):
        rc, plan = self.plan(d)
        assert rc == 0, rc
        tgc.host_gemm(d, plan)

    def conv2d(self, x, weight, bias=None, *, x2=None, rowvec=None, rows_per_vec=0, residual=None):
        """ops.conv2d's description of the call (dense output and residual), through the restatement"""
        nimg, Hh, Ww, C1 = x.shape
        d = self.GemmDesc()
        d.M, d.N, d.K, d.batch0, d.batch1, d.alpha = nimg * Hh * Ww, weight.shape[0], 9 * weight.shape[3], 1, 1, 1.0
        d.a_mode, d.H, d.W, d.C1, d.C2, d.ks, d.stride = 1, Hh, Ww, C1, weight.shape[3] - C1, 3, 1
        out = torch.empty(nimg, Hh, Ww, d.N, dtype=H)
        d.A, d.A2, d.C, d.ldc = x.data_ptr(), x2.data_ptr() if x2 is not None else None, out.data_ptr(), d.N
        d.bias = bias.data_ptr() if bias is not None else None
        if rowvec is not None:
            d.rowvec, d.rows_per_vec = rowvec.data_ptr(), rows_per_vec
        if residual is not None:
            d.residual, d.ldr = residual.data_ptr(), d.N
        need = self.wino_workspace(d)
        assert need > 0 and int(self.lib().vsx_conv3x3_winograd_auto(ctypes.byref(d))) == 1
        ws = torch.empty(need // 2, dtype=H)
        u = self.winograd_weights(weight)
        assert self.winograd(d, u.data_ptr(), ws.data_ptr(), need) == wc.VSX_OK
        return out, 1


class LibraryImpl(HostImpl):
    """the library's own entry point: only for descriptions it must refuse before any launch"""

    def winograd(self, d, u_ptr, ws_ptr, ws_bytes):
        return int(self.lib().vsx_conv3x3_winograd_f16(ctypes.byref(d), ctypes.c_void_p(u_ptr), ctypes.c_void_p(ws_ptr), ws_bytes, None))


HOST = HostImpl()


# ---- 1. the restatement passes every case of both classes; 2. the precondition of Inputs E ----
@pytest.mark.parametrize('c', wc.ENTRY_CASES, ids=wc.case_id)
def test_restatement_passes_the_rule(c):
    n = len(wc.FIGURES)
    fig = wc.run_case(HOST, CPU, c)
    del wc.FIGURES[n:]
    if c['cls'] == 'E':
        assert fig['ties'] > 0 or 'b' not in c['epi'] or c['M'] * c['N'] < 64, (c['name'], 'no tie among the exact results')


@pytest.mark.parametrize('c', wc.WRAPPER_CASES, ids=wc.case_id)
def test_wrapper_cases_on_the_restatement(c):
    n = len(wc.FIGURES)
    wc.run_wrapper(HOST, CPU, c)
    del wc.FIGURES[n:]


def test_exact_inputs_are_fp16_exact_at_every_stage():
    for c in wc.ENTRY_CASES + wc.WRAPPER_CASES:
        if c['cls'] == 'E':
            v, u, mt = wc.exact_stages(c, wc.make_inputs(c))
            assert float(mt.abs().max()) < 512 and float(v.abs().max()) <= 4 * c['amp'][0] and float(u.abs().max()) <= 2.25 * c['amp'][1]
    with pytest.raises(AssertionError):                   # ... and the assertion bites: [-3, 3] x [-2, 2] at 1280 channels is not exact
        c = dict(wc.BY_NAME['deep-level-channels-E-1x4x4-1280+0-to64-bvr-rpvHW-ldc+0'], amp=(3, 2))
        wc.exact_stages(c, wc.make_inputs(c))


def test_the_table_covers_what_it_claims():
    cases = wc.ENTRY_CASES
    E = [c for c in cases if c['cls'] == 'E']
    assert {c['tiles'] for c in E} >= {1, 127, 128, 129}
    assert {(c['H'], c['W']) for c in E} >= {(2, 2), (2, 16), (16, 2), (4, 6), (6, 4)} and {c['nimg'] for c in E} == {1, 2, 3}
    for per in ('C1', 'N'):                                # threads per transform against the 256-thread workgroup
        threads = {c['tiles'] * ((c['C1'] + c['C2']) if per == 'C1' else c['N']) // 8 for c in E}
        assert min(threads) < 256 and 256 in threads and any(t % 256 == 1 and t > 256 for t in threads), per
    assert {c['C1'] for c in E if not c['C2']} >= {8, 64, 72, 136} and {c['N'] for c in E} >= {8, 24, 64, 72}
    for cls in 'ER':
        assert {(c['C1'], c['C2']) for c in cases if c['cls'] == cls} >= {(64, 128), (128, 64)}, cls
    assert any(c['C1'] + c['C2'] >= 640 and c['amp'] == (1, 1) for c in E)
    assert {c['epi'] for c in E} >= {'', 'b', 'v', 'r', 'bv', 'br', 'vr', 'bvr'}
    for c in E:
        if c['edge'] == 'rows-per-vec':
            assert c['rpv'] in (c['H'] * c['W'], 2 * c['H'] * c['W'], c['W'], 3, 1)
    assert {c['rpv'] for c in E if c['edge'] == 'rows-per-vec' and c['W'] == 6} == {24, 48, 6, 3, 1}
    assert {c['pad'] for c in cases} == {0, 8, 16} and all(wc.RPAD[p] != p for p in wc.RPAD)
    assert any(c['pad11'] for c in E) and any(c['res_scale'] for c in cases if c['cls'] == 'R')
    assert {c['opts'].get('gemm_pp') for c in wc.WRAPPER_CASES} == {0, 1}
    assert all(c['C2'] and 'v' in c['epi'] and 'r' in c['epi'] for c in wc.WRAPPER_CASES)
    assert len(wc.REFUSALS) == 11 and sum(r[3] == wc.VSX_E_WORKSPACE for r in wc.REFUSALS) == 1


def test_the_batched_launch_stays_on_the_tile_kernels_under_every_gemm_pp():
    """The plan query makes no HIP call.  plan_gemm (csrc/gemm.hip) gives the persistent and the weight-stationary kernels
    launches without a batch only, so the sixteen GEMMs run on the workgroup-per-tile kernels whatever "gemm_pp" says: the
    cases under gemm_pp 0 and 1 pin that the option changes no bit, not a second back end.  Should the planner ever hand a
    batch to another family, this fails and the table needs a case aimed at it."""
    for c in wc.ENTRY_CASES + wc.WRAPPER_CASES:
        for pp in (0, 1, 2):
            with wc.options(HOST, dict(c['opts'], gemm_pp=pp)):
                assert HOST.batched_family(c) == gc.TILE, (c['name'], pp)


# ---- 3. the mutants ----
MUTANTS = {
    'padding_clamped_to_the_border': 'one-tile-all-taps-outside-the-interior-are-padding-E-1x2x2-8+0-to8-bvr-rpvHW-ldc+0',
    'window_origin_2ti': 'one-tile-all-taps-outside-the-interior-are-padding-E-1x2x2-8+0-to8-bvr-rpvHW-ldc+0',
    'th_tw_swapped': 'wider-than-tall-E-3x4x6-64+0-to64-bvr-rpvHW-ldc+8',
    'x2_with_c1_stride': 'two-sources-E-3x4x6-64+128-to24-bvr-rpvHW-ldc+8',
    'bt_row_sign': 'one-tile-per-image-E-3x2x2-8+0-to8-bvr-rpv2HW-ldc+8',
    'xi_transposed_in_v': 'taller-than-wide-one-tile-column-E-1x6x2-72+0-to24-bvr-rpvHW-ldc+0',
    'v_rounded_after_the_column_pass': 'resnet-conv1-R-3x4x6-64+0-to64-bv-rpvHW-ldc+0',
    'output_summed_in_fp16': 'resnet-conv1-R-3x4x6-64+0-to64-bv-rpvHW-ldc+0',
    'k_tail_dropped': 'K72-E-1x4x6-72+0-to8-bvr-rpvHW-ldc+8',
    'q_halves_swapped': 'one-tile-all-taps-outside-the-interior-are-padding-E-1x2x2-8+0-to8-bvr-rpvHW-ldc+0',
    'rowvec_once_per_tile': 'rows-per-vec-E-3x4x6-8+0-to24-bv-rpvW-ldc+16',
    'residual_with_ldc': 'one-tile-row-wide-E-1x2x16-8+0-to8-br-ldc+16',
    'bias_after_the_rounding': 'bias-ties-E-3x4x6-64+0-to64-bvr-rpv1-ldc+0',
    'store_n_plus_8_columns': 'one-tile-row-wide-E-1x2x16-8+0-to8-br-ldc+16',
    'mt_one_tile_past_the_end': 'one-tile-all-taps-outside-the-interior-are-padding-E-1x2x2-8+0-to8-bvr-rpvHW-ldc+0',
    'input_last_partial_workgroup_dropped': '257-threads-in-and-out-E-1x2x514-8+0-to8-br-ldc+16',
    'output_last_partial_workgroup_dropped': '513-threads-in-257-out-E-1x2x514-16+0-to8-bv-rpv1-ldc+0',
}


@pytest.mark.parametrize('mut', sorted(MUTANTS))
def test_mutant_is_rejected_by_its_named_case(mut):
    c = wc.BY_NAME[MUTANTS[mut]]
    n = len(wc.FIGURES)
    with pytest.raises(AssertionError):
        wc.run_case(HostImpl(mut), CPU, c)
    del wc.FIGURES[n:]
    wc.run_case(HOST, CPU, c)                     # ... and the same case passes without it
    del wc.FIGURES[n:]


def test_mutants_show_in_the_stage_they_break():
    """the harness says WHICH stage broke: a mutant of one transform leaves the figures of the other stages at zero"""
    def figures(mut):
        n = len(wc.FIGURES)
        try:
            wc.run_case(HostImpl(mut), CPU, wc.BY_NAME[MUTANTS[mut]])
        except AssertionError:
            pass
        fig = wc.FIGURES[n]
        del wc.FIGURES[n:]
        return fig
    f = figures('bt_row_sign')
    assert f['v_mismatches'] > 0 and f['mt_mismatches'] > 0 and f['y_mismatches'] == 0 and f['y_mismatches_fp64'] > 0
    f = figures('k_tail_dropped')
    assert f['v_mismatches'] == 0 and f['mt_mismatches'] > 0 and f['y_mismatches'] == 0 and f['y_mismatches_fp64'] > 0
    f = figures('q_halves_swapped')
    assert f['v_mismatches'] == 0 and f['mt_mismatches'] == 0 and f['y_mismatches'] > 0
    f = figures('v_rounded_after_the_column_pass')
    assert f['v_mismatches'] > 0 and f['y_mismatches'] == 0 and f['rel_l2'] < wc.REL_L2_BOUND      # (the whole-tensor bound alone misses it)
    f = figures('output_summed_in_fp16')
    assert f['v_mismatches'] == 0 and f['y_mismatches'] > 0 and f['rel_l2'] < wc.REL_L2_BOUND


def test_double_rounding_shows_in_the_tie_case():
    """why the bias range is what it is: with acc + bias beyond 2048 a bias added after the rounding is no rare event"""
    c = wc.BY_NAME[MUTANTS['bias_after_the_rounding']]
    n = len(wc.FIGURES)
    with pytest.raises(AssertionError):
        wc.run_case(HostImpl('bias_after_the_rounding'), CPU, c)
    fig = wc.FIGURES[n]
    del wc.FIGURES[n:]
    assert fig['y_mismatches'] > 0.05 * fig['elements'] and fig['ties'] > 0.2 * fig['elements'], fig


def test_the_sampled_check_of_the_large_index_case_on_a_small_stand_in():
    """winograd_case.run_large at a shape the CPU can hold: the restatement passes it, a mutant of each stage does not, and the
    sample holds the first and last tiles and the corners of the last image"""
    n = len(wc.FIGURES)
    fig = wc.run_large(HOST, CPU, wc.SMALL_STAND_IN)
    assert fig['sampled_tiles'] == 2 * 2 * 3                # all twelve tiles of the stand-in: the 64 random draws cover them
    for mut in ('window_origin_2ti', 'k_tail_dropped', 'q_halves_swapped', 'mt_one_tile_past_the_end'):
        with pytest.raises(AssertionError):
            wc.run_large(HostImpl(mut), CPU, dict(wc.SMALL_STAND_IN, C=72) if mut == 'k_tail_dropped' else wc.SMALL_STAND_IN)
    del wc.FIGURES[n:]
    s = wc.large_sample(wc.LARGE).tolist()
    th, tw, tiles = wc.LARGE['H'] // 2, wc.LARGE['W'] // 2, wc.LARGE['nimg'] * wc.LARGE['H'] * wc.LARGE['W'] // 4
    assert {0, tiles - 1, tiles - th * tw, tiles - th * tw + tw - 1, tiles - tw}.issubset(s) and len(s) >= 64
    assert wc.LARGE['nimg'] * wc.LARGE['H'] * wc.LARGE['W'] * wc.LARGE['C'] == 2 ** 31 - 2 ** 20          # one W step below the form's limit
    d = wc.batched_desc(HOST, dict(C1=wc.LARGE['C'], C2=0, N=wc.LARGE['N'], tiles=tiles))
    assert 15 * d.a_bs0 > 2 ** 31 and d.M * d.lda * 2 < 2 ** 31                                          # the batch offsets pass 2^31, a slice does not


# ---- 4. the refusals ----
@pytest.mark.parametrize('r', wc.REFUSALS, ids=lambda r: r[0])
def test_refusals_one_step_outside_the_supported_set(r):
    wc.run_refusal(HOST, CPU, r)
    wc.run_refusal(LibraryImpl(), CPU, r)             # the library itself: refused before any launch, nothing written


def test_a_refusal_that_writes_is_caught():
    class Writes(HostImpl):
        def winograd(self, d, u_ptr, ws_ptr, ws_bytes):
            _mem(ws_ptr, 8)[:] = 0
            return wc.VSX_E_UNSUPPORTED
    with pytest.raises(AssertionError):
        wc.run_refusal(Writes(), CPU, wc.REFUSALS[0])


def test_options_are_back_where_they_were():
    from videoswap_amd import ops
    import os
    for name, default, env in (('gemm_pp', 1, 'VSX_GEMM_PP'), ('conv_winograd', 1, 'VSX_CONV_WINOGRAD'), ('tile_tune', 0, 'VSX_TUNE_TILE')):
        assert ops.get_option(name) == (default if os.environ.get(env) is None else int(os.environ[env])), name
