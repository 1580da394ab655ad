"""The cases and the rule of tests/gemm_case.py, proven on the CPU before a GPU sees them.

1. A restatement of vsx_gemm_f16 ON THE DESCRIPTOR runs in the kernels' place: it reads and writes the host memory the descriptor
   points at (so a stray store lands in the guard band, as a kernel's would), sums K in 64-wide slabs in fp32, slice by slice
   where the plan splits, in tap order for a convolution, and applies the epilogue in the documented order with one rounding.  It
   is written with index arithmetic (the kernels' way); the references of gemm_case.py use padding, slicing and matmul in fp64.  It
   passes every case of both classes: bit-equal on Inputs E, inside the rule on Inputs R, every R case by name.
2. The plan every case names is the plan vsx_gemm_plan answers: the query makes no HIP call, so the whole table is checked here.
3. Every mutant of MUTANTS, planted in the restatement, is rejected by the case named next to it.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import gemm_case as gc
import host_emulation

CPU = 'cpu'
H = torch.float16


def _mem(ptr, dtype, count):
    """`count` elements of host memory at `ptr`, as a tensor that shares it"""
    size = torch.empty((), dtype=dtype).element_size()
    return torch.frombuffer((ctypes.c_char * (count * size)).from_address(ptr), dtype=dtype, count=count)


def _conv_a(d, mut):
    """[M, K] fp16: the implicit im2col by index arithmetic (row m -> image, ho, wo; tap (kh, kw); source; channel)"""
    ups = 1 if d.upsample else 0
    Hs, Ws = (d.H // 2, d.W // 2) if ups else (d.H, d.W)
    lo, hi = (d.ks // 2, d.ks // 2) if d.pad_lo < 0 else (d.pad_lo, d.pad_hi)
    if mut == 'pad01_swapped':
        lo, hi = hi, lo
    Ho, Wo = (d.H + lo + hi - d.ks) // d.stride + 1, (d.W + lo + hi - d.ks) // d.stride + 1
    m = torch.arange(d.M)
    img, rem = m // (Ho * Wo), m % (Ho * Wo)
    org = 1 if mut == 'stride2_origin' and d.stride == 2 else 0
    h0, w0 = (rem // Wo) * d.stride - lo + org, (rem % Wo) * d.stride - lo + org
    npix = (d.M // (Ho * Wo)) * Hs * Ws
    srcs = [_mem(d.A, H, npix * d.C1).view(npix, d.C1)]
    if d.C2:
        srcs.append(_mem(d.A2, H, npix * d.C2).view(npix, d.C2))
        if mut == 'wrong_source' and d.C1 >= d.C2:
            srcs[1] = srcs[0][:, :d.C2]
    cols = []
    for kh in range(d.ks):
        for kw in range(d.ks):
            h, w = h0 + kh, w0 + kw
            ok = (h >= 0) & (h < d.H) & (w >= 0) & (w < d.W)
            if ups:
                hs, ws = ((h + 1) >> 1, (w + 1) >> 1) if mut == 'upsample_round' else (h >> 1, w >> 1)
                hs, ws = hs.clamp(max=Hs - 1), ws.clamp(max=Ws - 1)
            else:
                hs, ws = h, w
            flat = (img * Hs + hs) * Ws + ws
            if mut == 'left_pad_wraps':         # the column bound is not checked on the left: w = -1 is the pixel in front of the row
                ok = (h >= 0) & (h < d.H) & (w < d.W) & (flat >= 0)
            for x in srcs:
                v = x[flat.clamp(0, npix - 1)].clone()
                v[~ok] = 0
                cols.append(v)
    return torch.cat(cols, dim=1)


def host_gemm(d, plan, mut=None):
    M, N, K = d.M, d.N, d.K
    geglu = bool(d.geglu)
    cols = 2 * N if geglu else N
    b1, nb = d.batch1, d.batch0 * d.batch1
    BM, BN = plan['BM'], plan['BN']
    nk = (K + gc.BK - 1) // gc.BK
    splits = plan['splits']
    slices = [(s * plan['nk_per'], min(nk, (s + 1) * plan['nk_per'])) for s in range(splits)] if splits > 1 else [(0, nk)]
    if mut == 'last_slice_dropped' and splits > 1:
        slices = slices[:-1]
    subpix = d.a_mode == 1 and d.upsample == 2
    alpha = 1.0 if mut == 'alpha_dropped' else d.alpha
    m_idx = torch.arange(M)
    for z in range(nb):
        z0, z1 = z // b1, z % b1
        if d.a_mode == 0:
            A = torch.as_strided(_mem(d.A, H, z0 * d.a_bs0 + z1 * d.a_bs1 + M * d.lda), (M, min(K + 8, d.lda)), (d.lda, 1), z0 * d.a_bs0 + z1 * d.a_bs1)
        elif subpix:
            A = None
        else:
            A = _conv_a(d, mut)
        boff = z0 * d.b_bs0 + z1 * d.b_bs1
        brows = 4 * cols if subpix else cols
        B = torch.as_strided(_mem(d.B, H, boff + brows * d.ldb), (brows, min(K + 8, d.ldb)), (d.ldb, 1), boff)
        if geglu and mut == 'geglu_g_offset_cols':
            B = torch.cat([B[:N], B[:N]])          # row N + n + N of a 2 N-row matrix, wrapped: the h row again
        if subpix:
            acc = _subpixel_acc(d, B, cols)
        else:
            parts = []
            for k0, k1 in slices:
                acc = torch.zeros(M, cols)
                for kt in range(k0, k1):
                    lo, hi = kt * gc.BK, min(K, (kt + 1) * gc.BK)
                    last = kt == nk - 1 and K % gc.BK != 0
                    if last and mut == 'pad_unmasked' and d.a_mode == 0:
                        hi = K + 8
                    blk = A[:, lo:hi].float() @ B[:, lo:hi].float().t()
                    if last and mut == 'ktail_dropped':            # tile (0, 0) stops 8 columns early
                        blk[:BM, :BN] = A[:BM, lo:hi - 8].float() @ B[:BN, lo:hi - 8].float().t()
                    acc = acc + blk
                parts.append(acc)
            acc = parts[0]
            for p in parts[1:]:
                acc = acc + p
        acc = acc * alpha
        n_idx = torch.arange(cols)
        if d.rowscale:
            rs = _mem(d.rowscale, torch.float32, 2 * M).view(M, 2)
            cv = _mem(d.colvec, torch.float32, cols)
            acc = rs[:, :1] * acc + rs[:, 1:] * cv[None, :]
        if d.bias:
            b = _mem(d.bias, H, cols)[n_idx % BN if mut == 'bias_tile_local' else n_idx]
            acc = (acc.to(H) + b[None, :]).float() if mut == 'bias_fp16' else acc + b.float()[None, :]
        if geglu:
            g = acc[:, N:]
            acc = acc[:, :N] * (F.gelu(g, approximate='tanh') if mut == 'tanh_gelu' else 0.5 * g * (1.0 + torch.erf(g * 0.7071067811865476)))
        if d.rowvec:
            rpv = max(d.rows_per_vec, 1)
            vi = (m_idx - m_idx % 32) // rpv if mut == 'rowvec_block_start' else m_idx // rpv
            acc = acc + _mem(d.rowvec, H, ((M + rpv - 1) // rpv) * N).view(-1, N)[vi].float()
        if d.residual:
            if mut == 'round_before_residual':
                acc = acc.to(H).float()
            ldr = d.ldc if mut == 'ldc_for_residual' else d.ldr
            roff = z0 * d.r_bs0 + z1 * d.r_bs1
            acc = acc + torch.as_strided(_mem(d.residual, H, roff + M * max(d.ldr, ldr)), (M, N), (ldr, 1), roff).float()
        out = acc.to(H)
        if d.c_mode == 0:
            coff = z0 * d.c_bs0 + z1 * d.c_bs1
            width = N + 1 if mut == 'store_into_column_pad' and d.ldc > N else N
            C = torch.as_strided(_mem(d.C, H, coff + (M - 1) * d.ldc + width), (M, width), (d.ldc, 1), coff)
            C[:, :N] = out
            if width > N:
                C[:, N] = 0
        else:
            rpi = d.c_rows_per_img
            img = (m_idx - m_idx % 4) // rpi if mut == 'vt_image_of_the_quad' else m_idx // rpi
            at = (img * d.c_img_stride + (m_idx - img * rpi))[:, None] + torch.arange(N)[None, :] * d.ldc
            C = _mem(d.C, H, int(at.max()) + 1)
            C[at.reshape(-1)] = out.reshape(-1)
        if d.rowstats:
            np_ = d.rowstats_parts
            st = _mem(d.rowstats, torch.float32, M * np_ * 2).view(M, np_, 2)
            for p, chunk in enumerate(torch.tensor_split(out.float(), np_, dim=1)):
                st[:, p, 0], st[:, p, 1] = chunk.sum(1), chunk.pow(2).sum(1)


def _subpixel_acc(d, B, N):
    """upsample = 2: output pixel (2 i + ph, 2 j + pw) = a pad-1 3x3 window on the SOURCE at (i, j) with the class matrix 2 ph + pw"""
    Hs, Ws, C = d.H // 2, d.W // 2, d.C1
    nimg = d.M // (d.H * d.W)
    x = _mem(d.A, H, nimg * Hs * Ws * C).view(nimg, Hs, Ws, C).float()
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    win = torch.cat([xp[:, kh:kh + Hs, kw:kw + Ws, :] for kh in range(3) for kw in range(3)], dim=-1)        # [nimg, Hs, Ws, 9 C]
    out = torch.zeros(nimg, d.H, d.W, N)
    for ph in (0, 1):
        for pw in (0, 1):
            out[:, ph::2, pw::2, :] = win @ B[(2 * ph + pw) * N:(2 * ph + pw + 1) * N, :d.K].float().t()
    return out.reshape(d.M, N)


class HostLN:
    def __init__(self, x, gamma, beta, eps):
        self.x, self.gamma, self.beta, self.eps = x, gamma, beta, eps


class HostImpl(gc.LibQueries):
    """the restatement behind the interface the runners use; `mut` plants one mutant"""
    DeferredLN = HostLN

    def __init__(self, mut=None):
        super().__init__()
        self.mut = mut

    def gemm(self, d):
        rc, plan = self.plan(d)
        assert rc == 0, rc
        host_gemm(d, plan, self.mut)

    def _desc(self, x, w, b, out, ldc):
        d = self.GemmDesc()
        d.M, d.K = x.shape
        d.N = w.shape[0]
        d.batch0 = d.batch1 = 1
        d.alpha = 1.0
        d.A, d.lda, d.B, d.ldb, d.C, d.ldc = x.data_ptr(), d.K, w.data_ptr(), d.K, out.data_ptr(), ldc
        d.bias = b.data_ptr()
        return d

    def _fold(self, d, ln, w, b):
        """ops._ln_folded and DeferredLN.stats, restated"""
        w32 = w.float()
        wf = (w32 * ln.gamma.float()[None, :]).to(H)
        c1, c2 = wf.float().sum(1).contiguous(), (w32 @ ln.beta.float() + b.float()).to(H)
        var, mean = torch.var_mean(ln.x.float(), dim=-1, unbiased=False)
        rstd = (var + ln.eps).rsqrt()
        st = torch.stack([rstd, -rstd * mean], dim=1).contiguous()
        d.B, d.bias, d.rowscale, d.colvec = wf.data_ptr(), c2.data_ptr(), st.data_ptr(), c1.data_ptr()
        return wf, c1, c2, st

    def linear(self, x, weight, bias=None, residual=None, geglu=False, out=None):
        if not isinstance(x, HostLN):
            return host_emulation.linear(x, weight, bias, residual=residual, geglu=geglu, out=out)
        y = torch.empty(x.x.shape[0], weight.shape[0], dtype=H)
        d = self._desc(x.x, weight, bias, y, weight.shape[0])
        keep = self._fold(d, x, weight, bias)
        if d.K >= 768:
            ws = torch.zeros(max(self.workspace(d), 4) // 4, dtype=torch.float32)
            d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel() * 4
        self.gemm(d)
        del keep
        return y

    def linear_vt(self, x, weight, bias, rows_per_img, ldvt=None):
        if not isinstance(x, HostLN):
            return host_emulation.linear_vt(x, weight, bias, rows_per_img, ldvt=ldvt)
        M, N = x.x.shape[0], weight.shape[0]
        ldvt = ldvt or gc.round_up(rows_per_img, 8)
        vt = torch.zeros(M // rows_per_img, N, ldvt, dtype=H)
        d = self._desc(x.x, weight, bias, vt, ldvt)
        d.c_mode, d.c_rows_per_img, d.c_img_stride = 1, rows_per_img, N * ldvt
        keep = self._fold(d, x, weight, bias)
        self.gemm(d)
        del keep
        return vt

    def conv2d_form(self, subpixel, x, w, b, upsample):
        return host_emulation.conv2d(x, w, b, upsample=upsample)


HOST = HostImpl()


# ---- 1. the restatement passes every case of both classes ----
@pytest.mark.parametrize('c', [c for c in gc.ALL_CASES if c['cls'] == 'E'], ids=gc.case_id)
def test_restatement_is_bit_equal_on_exact_inputs(c):
    gc.run_case(HOST, CPU, c)


@pytest.mark.parametrize('name', gc.R_NAMES)
def test_restatement_is_inside_the_rule_on_rounded_inputs(name):
    gc.run_case(HOST, CPU, gc.BY_NAME[name])


@pytest.mark.parametrize('name', gc.WRAPPER_RUNS)
def test_wrapper_runs_on_the_stand_ins(name):
    gc.run_wrapper(HOST, CPU, name)


# ---- 2. the plans, for the whole table; the refusals; the options come back ----
def test_every_case_meets_the_plan_it_names():
    before = {k: HOST.get_option(k) for k in gc.BASE_OPTS}
    seen = set()
    for c in gc.ALL_CASES + gc.REFUSALS:
        with gc.options(HOST, c['opts']):
            plan = gc.assert_plan(HOST, gc.build(c, CPU, HOST))
            seen.add((plan['family'], plan['BM'], plan['BN'], plan['deep'], plan['splits'] > 1))
    assert before == {k: HOST.get_option(k) for k in gc.BASE_OPTS}
    # every kernel instance is met: the six tiles, the deep ring, split-K, both persistent tiles, the weight-stationary kernel
    for want in [(gc.TILE, bm, bn, 0, False) for bm, bn in gc.FORCED_TILE.values()] + [(gc.TILE, 128, 160, 1, False), (gc.TILE, 128, 320, 0, True),
                                                                                       (gc.PP256, 256, 320, 0, False), (gc.PP128, 128, 320, 0, False),
                                                                                       (gc.WS, 32, 320, 0, False)]:
        assert want in seen, want


@pytest.mark.parametrize('c', gc.REFUSALS, ids=gc.case_id)
def test_refusals_just_below_the_smallest_eligible_shape(c):
    assert gc.run_case(HOST, CPU, c) is None


def test_a_forced_split_never_leaves_a_slice_empty():
    """every forced count against every slab count: the slices of the plan cover the slabs and the last one has at least one"""
    d = HOST.GemmDesc()
    d.M, d.N, d.batch0, d.batch1, d.alpha, d.ldc = 100, 320, 1, 1, 1.0, 320
    d.A = d.B = d.C = d.workspace = 0x10000
    for s in range(2, 16):
        for nk in range(1, 40):
            d.K = d.lda = d.ldb = 64 * nk
            with gc.options(HOST, dict(tile_tune=256 * s)):
                d.workspace_bytes = HOST.workspace(d)
                rc, plan = HOST.plan(d)
            assert rc == 0 and plan['splits'] <= min(s, nk), (s, nk, plan)
            if plan['splits'] > 1:
                assert (plan['splits'] - 1) * plan['nk_per'] < nk <= plan['splits'] * plan['nk_per'], (s, nk, plan)


def test_the_table_covers_what_it_claims():
    cases = gc.ALL_CASES
    assert {c['pad'] for c in gc.TILE_CASES} == {0, 1, 4, 8}
    assert {c['alpha'] for c in cases} == {1.0, 0.25, 2.0}
    assert all(n in gc.BY_NAME for n in gc.R_NAMES) and all('g' not in c['epi'] or c['cls'] == 'R' for c in cases)
    pads = {(c['conv'][8], c['conv'][9]) for c in gc.CONV_CASES}
    assert {(-1, -1), (0, 1), (1, 0), (0, 0), (2, 2)} <= pads
    assert {c['conv'][3] for c in gc.CONV_CASES} >= {8, 24, 64, 72, 128}
    assert {(c['conv'][1], c['conv'][2]) for c in gc.CONV_CASES} >= {(1, 1), (1, 5), (2, 2), (3, 5), (5, 3), (7, 9), (8, 8), (16, 16), (32, 32)}
    assert {c['opts'].get('pp_sched', 0) for c in gc.CONV_CASES} >= {0, 4, 16, 32}
    assert any(c['conv'][5] == 1 and c['conv'][6] == 2 for c in gc.CONV_CASES)
    assert any(c['M'] == 33280 for c in gc.PP_CASES) and max(c['M'] * c['N'] for c in cases) == 33280 * 640


# ---- 3. the mutants ----
MUTANTS = {
    'ktail_dropped': 'tile6-ladder-65x72x72',
    'pad_unmasked': 'tile6-ladder-65x72x72',
    'bias_tile_local': 'tile6-65x200x8-b-pad8',
    'rowvec_block_start': 'tile2-epi-257x320x72-bv48',
    'ldc_for_residual': 'tile6-ladder-65x72x72',
    'round_before_residual': 'tile6-ladder-65x72x72',
    'bias_fp16': 'tile6-ladder-65x72x72',
    'tanh_gelu': 'tile2-epi-257x160x72-bg',
    'geglu_g_offset_cols': 'tile2-epi-257x160x72-bg',
    'last_slice_dropped': 'split2-100x640x136-br-pad0',
    'left_pad_wraps': 'conv-tile-3x5x3-24+0-k3s1-to40-bvr-ldc+1',
    'upsample_round': 'conv-tile-3x3x5-72+0-k3s1-up-to40-bvr-ldc+1',
    'stride2_origin': 'conv-tile-3x7x9-72+0-k3s2-to40-br-ldc+1',
    'pad01_swapped': 'conv-tile-3x7x9-24+0-k3s2-pad01-to40-bvr-ldc+4',
    'wrong_source': 'conv-tile-3x5x3-64+64-k3s1-to40-bvr',
    'vt_image_of_the_quad': 'tile6-vt-135x72x72-bt5',
    'store_into_column_pad': 'tile6-epi-130x72x72-br',
    'alpha_dropped': 'tile6-epi-130x72x72-br',
}


@pytest.mark.parametrize('mut', sorted(MUTANTS))
def test_mutant_is_rejected_by_its_named_case(mut):
    c = gc.BY_NAME[MUTANTS[mut]]
    n = len(gc.FIGURES)
    with pytest.raises(AssertionError):
        gc.run_case(HostImpl(mut), CPU, c)
    del gc.FIGURES[n:]
    gc.run_case(HOST, CPU, c)                     # ... and the same case passes without it
    del gc.FIGURES[n:]


def test_double_rounding_shows_in_a_quarter_of_the_elements():
    """why the bias range is what it is: with acc + bias beyond 2048 a second rounding is no rare event"""
    c = gc.BY_NAME['tile6-ladder-65x72x72']
    for mut in ('round_before_residual', 'bias_fp16'):
        with gc.options(HOST, c['opts']):
            pb = gc.build(c, CPU, HOST)
            HostImpl(mut).gemm(pb.d)
            got, want = pb.cbuf[pb.cidx], gc.chain(pb, torch.float64).to(H)
        frac = float((got != want).float().mean())
        assert 0.1 < frac < 0.5, (mut, frac)


def test_one_lost_tail_shows_as_that_tile_only():
    c = gc.BY_NAME['tile6-ladder-65x72x72']
    with gc.options(HOST, c['opts']):
        pb = gc.build(c, CPU, HOST)
        HostImpl('ktail_dropped').gemm(pb.d)
        diff = pb.cbuf[pb.cidx] != gc.chain(pb, torch.float64).to(H)
    assert bool(diff[0, :64, :64].any()) and not bool(diff[0, 64:].any()) and not bool(diff[0, :, 64:].any())
