"""Tensor-level wrappers over the libvsx C ABI.

PyTorch is used for device memory and the HIP stream only: every function here takes fp16 CUDA
(ROCm) tensors, hands raw pointers + the current stream to a hand-written gfx950 kernel and
returns the output tensor.  There is no fallback implementation.
"""
import contextlib
import ctypes
import os
import weakref

import torch

from . import _lib
from ._lib import GemmDesc, check

_F16 = torch.float16


_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)


def _stream():
    """hipStream_t of torch's current stream (the raw-handle query is ~10x cheaper than building a Stream object;
    with ~700 launches per UNet call the difference is several ms of host time per forward)."""
    if _raw_stream is not None:
        return ctypes.c_void_p(_raw_stream(torch.cuda.current_device()))
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _chk(t, name, dtype=_F16):
    if t is None:
        return
    if not t.is_cuda:
        raise _lib.VsxError(f'{name}: expected a GPU tensor (the denoising path has no CPU implementation)')
    if t.dtype != dtype:
        raise _lib.VsxError(f'{name}: expected {dtype}, got {t.dtype}')
    if not t.is_contiguous():
        raise _lib.VsxError(f'{name}: expected a contiguous tensor, got strides {t.stride()}')


def round_up(x, m):
    return (x + m - 1) // m * m


# --------------------------------------------------------------------------------------------
# GEMM family
# --------------------------------------------------------------------------------------------
class FlopCounter:
    """Algorithmic FLOP (2 x MAC, true dimensions, no padding) of the MFMA kernels launched while enabled.  `gemm` counts what
    the launches multiply; `gemm_saved` what the reference's formulation would have multiplied on top of that (the five taps
    per output pixel that the sub-pixel form of the nearest-2x convolutions never computes)."""
    enabled = False
    gemm = 0.0
    gemm_saved = 0.0
    attention = 0.0

    @classmethod
    def reset(cls, enabled=True):
        cls.enabled, cls.gemm, cls.gemm_saved, cls.attention = enabled, 0.0, 0.0, 0.0


_split_ws = {}      # (device, stream) -> grow-only fp32 scratch for split-K partial sums (stream-ordered reuse)


# VSX_GEMM_LOG=<file>: one line per vsx_gemm_f16 launch (shape, loader mode, epilogue), in launch order — joined by
# tools/pmc_by_shape.py with rocprofv3's per-dispatch counters (the i-th GEMM dispatch is the i-th line).  Measurement only.
_gemm_log = None
if os.environ.get('VSX_GEMM_LOG'):
    _gemm_log = open(os.environ['VSX_GEMM_LOG'], 'w')


def gemm(desc, k_flop=None):
    """k_flop: the K the launch actually multiplies when that is not desc.K (sub-pixel form of the nearest-2x convolution)"""
    if _gemm_log is not None:
        _gemm_log.write(f'{desc.M} {desc.N} {desc.K} {desc.batch0 * desc.batch1} {desc.a_mode} {desc.ks} {desc.stride} '
                        f'{desc.upsample} {desc.C1} {desc.C2} {desc.H} {desc.W} {desc.geglu} {desc.c_mode} '
                        f'{1 if desc.residual else 0} {1 if desc.rowvec else 0} {1 if desc.bias else 0}\n')
        _gemm_log.flush()
    if FlopCounter.enabled:
        cols = desc.N * (2 if desc.geglu else 1)
        FlopCounter.gemm += 2.0 * desc.M * cols * (desc.K if k_flop is None else k_flop) * desc.batch0 * desc.batch1
        if k_flop is not None:
            FlopCounter.gemm_saved += 2.0 * desc.M * cols * (desc.K - k_flop) * desc.batch0 * desc.batch1
    lib = _lib.load()
    need = lib.vsx_gemm_workspace(ctypes.byref(desc)) if (desc.M <= 20480 and desc.K >= 768) else 0
    stream = _stream()
    if need > 0:
        # one scratch buffer per (device, stream): launches on one stream are ordered, two streams (or a graph capture
        # next to eager work) must not share partial sums
        key = (torch.cuda.current_device(), stream.value)
        ws = _split_ws.get(key)
        if ws is None or ws.numel() * 4 < need:
            ws = torch.empty((need + 3) // 4, dtype=torch.float32, device=f'cuda:{key[0]}')
            _split_ws[key] = ws
        desc.workspace, desc.workspace_bytes = ws.data_ptr(), ws.numel() * 4
    check(lib.vsx_gemm_f16(ctypes.byref(desc), stream), 'vsx_gemm_f16')


# --------------------------------------------------------------------------------------------
# LayerNorm folded into the Linear that consumes it (include/vsx.h: vsx_gemm_desc.rowscale / colvec)
# --------------------------------------------------------------------------------------------
LN_FUSE = os.environ.get('VSX_LN_FUSE', '1') != '0'     # 0: every LayerNorm runs as its own kernel (A/B runs)


# VSX_ROW_STATS_PRODUCER=0: LayerNorm row statistics always by the standalone pass (A/B runs)
ROW_STATS_FROM_PRODUCER = os.environ.get('VSX_ROW_STATS_PRODUCER', '1') != '0'
ROW_STATS_MAX_PARTS = 64           # vsx_row_stats_combine's limit (norm.hip): N <= 3200 on the persistent kernel's 6 parts per 320 columns


class DeferredLN:
    """A LayerNorm that has not been applied: `x` is the RAW activation, and the Linear(s) consuming the normalised tensor
    (attention.py:182,199,205 norm1/2/3 -> to_q / to_k / to_v / GEGLU; motion_module.py:213,219) apply it inside their
    GEMM through  LN(x) W^T + b = rstd * (x (W o gamma)^T) - rstd * mean * sum_k (W o gamma) + (beta W^T + b)  (+ pe W^T for
    the temporal positional encoding).  The normalised tensor is never written; the row statistics are computed once per
    DeferredLN (`stats()`), whatever the number of consumers.  Quacks like the tensor the processors expect as far as they
    use it (shape, reshape / view, dtype, device); `materialize()` is the ordinary kernel for anything else."""
    is_cuda = True
    requires_grad = False

    def __init__(self, x, gamma, beta, eps, pe=None, rows_per_frame=0, frames=0, frame_offset=0, _shared=None):
        self.x, self.gamma, self.beta, self.eps = x, gamma, beta, eps
        self.pe, self.rows_per_frame, self.frames, self.frame_offset = pe, rows_per_frame, frames, frame_offset
        self._shared = _shared if _shared is not None else {}          # stats / materialised tensor, shared by reshapes
        # partial row sums the producing GEMM hung on its output (they describe the ROWS: reshapes keep them)
        if 'row_parts' not in self._shared:
            self._shared['row_parts'] = getattr(x, '_vsx_rowparts', None)

    row_parts = property(lambda self: self._shared.get('row_parts'))

    shape = property(lambda self: self.x.shape)
    dtype = property(lambda self: self.x.dtype)
    device = property(lambda self: self.x.device)

    def dim(self):
        return self.x.dim()

    def numel(self):
        return self.x.numel()

    def contiguous(self):
        return self

    def _like(self, x):
        return DeferredLN(x, self.gamma, self.beta, self.eps, self.pe, self.rows_per_frame, self.frames, self.frame_offset,
                          self._shared)

    def reshape(self, *shape):
        return self._like(self.x.reshape(*shape))

    def view(self, *shape):
        return self._like(self.x.view(*shape))

    def stats(self):
        """[M, 2] fp32 = (rstd, -rstd * mean) per row, computed once: from the partial sums the GEMM that produced x
        wrote in its epilogue (`linear(..., row_stats=True)` hangs them on its output tensor) where there are any,
        otherwise by a pass over x (vsx_row_stats)"""
        st = self._shared.get('stats')
        if st is None:
            C = self.x.shape[-1]
            M = self.x.numel() // C
            st = torch.empty(M, 2, dtype=torch.float32, device=self.x.device)
            parts = self.row_parts
            if parts is not None and parts.shape[0] == M and ROW_STATS_FROM_PRODUCER:
                check(_lib.load().vsx_row_stats_combine(_p(parts), M, parts.shape[1], C, float(self.eps), _p(st), _stream()),
                      'vsx_row_stats_combine')
            else:
                check(_lib.load().vsx_row_stats(_p(self.x), M, C, float(self.eps), _p(st), _stream()), 'vsx_row_stats')
            self._shared['stats'] = st
        return st

    def materialize(self):
        y = self._shared.get('y')
        if y is None:
            y = _raw['layer_norm'](self.x.reshape(-1, self.x.shape[-1]), self.gamma, self.beta, self.eps, pe=self.pe,
                                   rows_per_frame=self.rows_per_frame, frames=self.frames, frame_offset=self.frame_offset)
            self._shared['y'] = y
        return y.view(self.x.shape)


# Operands derived from a weight, one protocol (`_derived`): key -> (stamp, weak references to the owners, *derived values)
_fold_cache = {}          # (id(weight), id(gamma)) -> (.., .., W o gamma, c1, c2, {pe products})
_subpixel_cache = {}      # id(weight) -> (.., .., [4, Cout, 3, 3, C] fp16)
_winograd_cache = {}      # id(weight) -> (.., .., [16, Cout, C] fp16)


def _derived(cache, key, owners, stamped, build):
    """cache[key], rebuilt (`build()` -> the derived values, under no_grad) when the address or version of a tensor in
    `stamped` has changed (LoRA merge / load_state_dict bump the version) or another object has taken the id of one of
    `owners`.  An entry lives exactly as long as owners[0], its weight tensor (a finalizer on the weight, registered once per
    weight object, evicts it: the fused-projection tensors that a LoRA merge rebuilds do not leave stale copies behind, and
    nothing is ever dropped while its weight — and therefore a graph captured over it — can still be used)."""
    stamp = tuple((t.data_ptr(), t._version) for t in stamped)
    hit = cache.get(key)
    if hit is None or hit[0] != stamp or any(r() is not o for r, o in zip(hit[1], owners)):
        fresh = hit is None or hit[1][0]() is not owners[0]
        with torch.no_grad():
            hit = (stamp, tuple(weakref.ref(o) for o in owners), *build())
        cache[key] = hit
        if fresh:
            weakref.finalize(owners[0], cache.pop, key, None)
    return hit


def fold_cache_tensors():
    """Every folded operand alive right now.  A captured HIP graph bakes their addresses into its kernel arguments:
    graphs.GraphCache keeps this list with the graph entry, so the memory outlives any eviction here."""
    out = []
    for hit in _fold_cache.values():
        out.extend((hit[2], hit[3], hit[4]))
        out.extend(hit[5].values())
    out.extend(hit[2] for hit in _subpixel_cache.values())
    out.extend(hit[2] for hit in _winograd_cache.values())
    return out


def _ln_folded(weight, bias, ln):
    """W' = W o gamma (fp16, the B operand), c1[n] = sum_k W'[n, k] (fp32), c2 = beta W^T + b (fp16, the epilogue bias) as
    entry[2], [3], [4] of `_fold_cache`; rebuilt when any of the parameters changes."""
    def build():
        w32 = weight.detach().reshape(weight.shape[0], -1).float()
        wf = (w32 * ln.gamma.detach().float()[None, :]).to(_F16).contiguous()
        c1 = wf.float().sum(1).contiguous()
        c2 = w32 @ ln.beta.detach().float()
        if bias is not None:
            c2 = c2 + bias.detach().float()
        return wf, c1, c2.to(_F16).contiguous(), {}
    return _derived(_fold_cache, (id(weight), id(ln.gamma)), (weight, ln.gamma),
                    (weight, ln.gamma, ln.beta) + ((bias,) if bias is not None else ()), build)


def _ln_pe_rows(hit, weight, ln, M):
    """pe W^T as the GEMM's row-vector term: [M / rows_per_frame, N] (row m takes frame (m / rows_per_frame) % frames)"""
    if ln.pe is None:
        return None, 0
    nblk = M // ln.rows_per_frame
    key = (ln.pe.data_ptr(), ln.pe._version, ln.frame_offset, ln.frames, nblk)
    rv = hit[5].get(key)
    if rv is None:
        with torch.no_grad():
            pe = ln.pe[ln.frame_offset:ln.frame_offset + ln.frames].float()
            rows = (pe @ weight.detach().reshape(weight.shape[0], -1).float().t()).to(_F16)        # [frames, N]
            rv = rows.repeat(nblk // ln.frames, 1).contiguous()
        if len(hit[5]) > 16:
            hit[5].clear()
        hit[5][key] = rv
    return rv, ln.rows_per_frame


def _bind_folded_ln(d, weight, bias, ln):
    """The LayerNorm `ln` applied inside the launch d describes: the folded weight and bias, the row statistics and c1, and the
    positional-encoding rows where there are any.  Returns what the caller keeps alive until the launch is enqueued."""
    hit = _ln_folded(weight, bias, ln)
    rv, rpv = _ln_pe_rows(hit, weight, ln, d.M)
    st = ln.stats()
    d.B = hit[2].data_ptr()
    d.bias = hit[4].data_ptr()
    d.rowscale, d.colvec = st.data_ptr(), hit[3].data_ptr()
    if rv is not None:
        d.rowvec, d.rows_per_vec = rv.data_ptr(), rpv
    return hit, rv, st


def linear(x, weight, bias=None, residual=None, geglu=False, out=None, row_stats=False):
    """y = x @ weight.T (+bias) (+residual); geglu: weight is [2N,K], y = h * gelu(g).

    x [..., K] -> [..., N].  Replaces nn.Linear / 1x1 conv / diffusers GEGLU.  `x` may be a DeferredLN: the LayerNorm is
    then applied inside the GEMM.  `row_stats`: a LayerNorm follows — where the launch can (vsx_gemm_rowstats_parts), its
    epilogue also writes per-row partial sums of the output, which then travel with the returned tensor
    (`y._vsx_rowparts`, picked up by layers.LayerNorm / DeferredLN.stats); a hint, never an obligation.
    """
    ln = x if isinstance(x, DeferredLN) else None
    if ln is not None:
        x = ln.x
    _chk(x, 'x'); _chk(weight, 'weight'); _chk(bias, 'bias'); _chk(residual, 'residual')
    K = x.shape[-1]
    M = x.numel() // K
    if weight.dim() == 4:  # 1x1 conv weight [N,K,1,1]
        weight = weight.reshape(weight.shape[0], weight.shape[1])
    n_rows = weight.shape[0]
    if weight.shape[1] != K:
        raise _lib.VsxError(f'linear: weight {tuple(weight.shape)} does not match input features {K}')
    N = n_rows // 2 if geglu else n_rows
    if out is None:
        out = torch.empty(*x.shape[:-1], N, dtype=_F16, device=x.device)
    d = GemmDesc()
    d.M, d.N, d.K = M, N, K
    d.batch0 = d.batch1 = 1
    d.A = x.data_ptr(); d.lda = K
    d.B = weight.data_ptr(); d.ldb = K
    d.C = out.data_ptr(); d.ldc = N
    d.bias = bias.data_ptr() if bias is not None else None
    keep = None
    if ln is not None:
        if ln.pe is not None and geglu:
            raise _lib.VsxError('linear: a positional encoding cannot be folded into a GEGLU projection')
        keep = _bind_folded_ln(d, weight, bias, ln)
    if residual is not None:
        if residual.numel() != M * N:
            raise _lib.VsxError('linear: residual shape mismatch')
        d.residual = residual.data_ptr(); d.ldr = N
    d.geglu = 1 if geglu else 0
    d.alpha = 1.0
    parts = None
    if row_stats and ln is None and not geglu and ROW_STATS_FROM_PRODUCER:
        nparts = int(_lib.load().vsx_gemm_rowstats_parts(ctypes.byref(d)))
        if 0 < nparts <= ROW_STATS_MAX_PARTS:      # (a hint, never an obligation: wider outputs take the stand-alone statistics pass)
            parts = torch.empty(M, nparts, 2, dtype=torch.float32, device=x.device)
            d.rowstats, d.rowstats_parts = parts.data_ptr(), nparts
    gemm(d)
    del keep
    if parts is not None:
        out._vsx_rowparts = parts
    return out


def linear_vt(x, weight, bias, rows_per_img, ldvt=None):
    """V^T projection: x [nimg*rows, K] -> VT [nimg, N, ldvt] with VT[i, n, r] = (x @ W.T)[i*rows + r, n].

    Feeds vsx_attention_f16 / attention_pv (V is consumed key-contiguous).  Columns >= rows of VT are left
    untouched (the consumers mask them).
    """
    ln = x if isinstance(x, DeferredLN) else None
    if ln is not None:
        x = ln.x
    _chk(x, 'x'); _chk(weight, 'weight'); _chk(bias, 'bias')
    K = x.shape[-1]
    M = x.numel() // K
    N = weight.shape[0]
    nimg = M // rows_per_img
    if ldvt is None:
        ldvt = round_up(rows_per_img, 8)
    vt = torch.empty(nimg, N, ldvt, dtype=_F16, device=x.device)
    if ldvt != rows_per_img:
        vt.zero_()
    d = GemmDesc()
    d.M, d.N, d.K = M, N, K
    d.batch0 = d.batch1 = 1
    d.A = x.data_ptr(); d.lda = K
    d.B = weight.data_ptr(); d.ldb = K
    d.C = vt.data_ptr(); d.ldc = ldvt
    d.c_mode = 1; d.c_rows_per_img = rows_per_img; d.c_img_stride = N * ldvt
    d.bias = bias.data_ptr() if bias is not None else None
    keep = None
    if ln is not None:
        if ln.pe is not None:
            raise _lib.VsxError('linear_vt: a positional encoding cannot be folded into the transposed V projection')
        keep = _bind_folded_ln(d, weight, bias, ln)
    d.alpha = 1.0
    gemm(d)
    del keep
    return vt


# VSX_CONV_SUBPIXEL=0: the nearest-2x convolutions always as nine taps on the upsampled image (A/B runs)
CONV_SUBPIXEL = os.environ.get('VSX_CONV_SUBPIXEL', '1') != '0'


def subpixel_weights(weight):
    """Sub-pixel form of `conv3x3(nearest_2x(x))` (Upsample3D, resnet.py:54,66): a 3x3 window on the upsampled image meets
    only 2 x 2 source pixels, so output pixel (2 i + ph, 2 j + pw) is a 2 x 2-tap convolution of the SOURCE with the filter
    rows / columns that land on the same source pixel added up (fp32 sums, rounded to fp16 once):
        ph = 0: source rows (i - 1, i) <- filter rows ({0}, {1, 2});   ph = 1: source rows (i, i + 1) <- ({0, 1}, {2})
    and the same along the columns.  Returns [4, Cout, 3, 3, C] (class = 2 ph + pw): the four taps of class (ph, pw) sit at
    window positions (ph.., pw..) of a plain pad-1 3x3 window on the source, the other five are zero and never read
    (include/vsx.h: vsx_gemm_desc.upsample = 2).  4 / 9 of the multiplications of the nine-tap form.  Cached per weight."""
    def build():
        w = weight.detach().float()                                   # [Cout, 3, 3, C]
        rows = {0: ((0, (0,)), (1, (1, 2))), 1: ((1, (0, 1)), (2, (2,)))}      # parity -> ((window tap, filter taps), ...)
        out = torch.zeros(4, *w.shape, dtype=torch.float32, device=w.device)
        for ph in (0, 1):
            for pw in (0, 1):
                for th, fh in rows[ph]:
                    for tw, fw in rows[pw]:
                        out[2 * ph + pw, :, th, tw] = sum(w[:, a, b] for a in fh for b in fw)
        return (out.to(_F16).contiguous(),)
    return _derived(_subpixel_cache, id(weight), (weight,), (weight,), build)[2]


# VSX_CONV_WINOGRAD (library option "conv_winograd"): 0 = the stride-1 3x3 convolutions always on the direct kernels,
# 1 = Winograd F(2x2, 3x3) where it measured faster (vsx_conv3x3_winograd_auto), 2 = wherever the form is supported (tests)
_WINO_G = ((1.0, 0.0, 0.0), (0.5, 0.5, 0.5), (0.5, -0.5, 0.5), (0.0, 0.0, 1.0))
_winograd_hold = [0]      # > 0: the gradient path is calling (videoswap_amd/autograd.py) — the training step keeps the direct kernels


@contextlib.contextmanager
def winograd_suspended():
    """The convolutions launched inside take the direct kernels whatever the option says: the adapter training step's forward
    and dgrad convolutions (flipped weight copies, sliced per source) are not part of what the Winograd form was measured on."""
    _winograd_hold[0] += 1
    try:
        yield
    finally:
        _winograd_hold[0] -= 1


def winograd_weights(weight):
    """U = G g G^T of Winograd F(2x2, 3x3) (include/vsx.h: vsx_conv3x3_winograd_f16) from a [Cout, 3, 3, C] weight: fp32
    arithmetic on the fp16 values, rounded to fp16 once, laid out [16, Cout, C] (xi = 4 a + b outermost: sixteen K-major
    GEMM operands).  16 / 9 of the weight's bytes.  Cached per weight."""
    def build():
        w = weight.detach().float()                                   # [Cout, 3, 3, C]
        G = torch.tensor(_WINO_G, dtype=torch.float32, device=w.device)
        u = torch.einsum('ar,orsc,bs->aboc', G, w, G)      # [4, 4, Cout, C]
        return (u.reshape(16, w.shape[0], w.shape[3]).to(_F16).contiguous(),)
    return _derived(_winograd_cache, id(weight), (weight,), (weight,), build)[2]


def _conv_form(d):
    """'subpixel' | 'winograd' | 'direct': the form `conv2d` launches the complete description d in.  The library decides, under
    its current options: the sub-pixel form of a nearest-2x convolution where vsx_gemm_f16 would take it (d.upsample is then
    left at 2), the Winograd form where vsx_conv3x3_winograd_auto says so and the gradient path is not calling.  The
    conditions in front of the first question only spare a call that cannot pass (the library checks them too)."""
    lib = _lib.load()
    if d.upsample and CONV_SUBPIXEL and d.ks == 3 and d.stride == 1 and d.pad_lo < 0 and d.pad_hi < 0 \
            and not (d.A2 or d.rowvec or d.residual):
        d.upsample = 2
        if lib.vsx_gemm_check(ctypes.byref(d)) == 0:
            return 'subpixel'
        d.upsample = 1
    if _winograd_hold[0] == 0 and lib.vsx_conv3x3_winograd_auto(ctypes.byref(d)) == 1:
        return 'winograd'
    return 'direct'


def _conv_winograd(d, weight, device):
    """The launch behind `conv2d` once the form is chosen: d is the direct path's description, complete."""
    lib = _lib.load()
    u = winograd_weights(weight)
    need = int(lib.vsx_conv3x3_winograd_workspace(ctypes.byref(d)))
    if need <= 0:
        raise _lib.VsxError('conv2d: the Winograd form does not take this convolution')
    ws = torch.empty(need // 2, dtype=_F16, device=device)     # V + Mt: the caching allocator's (under capture: the graph pool's)
    if FlopCounter.enabled:
        executed = 2.0 * d.M * d.N * (d.K // 9) * 4               # 16 products per 2 x 2 tile = 4 per output pixel
        FlopCounter.gemm += executed
        FlopCounter.gemm_saved += 2.0 * d.M * d.N * d.K - executed
    if _gemm_log is not None:
        _gemm_log.write(f'{d.M // 4} {d.N} {d.K // 9} 16 0 0 0 0 0 0 0 0 0 0 0 0 0\n')
        _gemm_log.flush()
    check(lib.vsx_conv3x3_winograd_f16(ctypes.byref(d), _p(u), _p(ws), need, _stream()), 'vsx_conv3x3_winograd_f16')


def conv2d(x, weight, bias=None, *, x2=None, stride=1, upsample=False, rowvec=None, rows_per_vec=0,
           residual=None, padding=None):
    """Channels-last conv as implicit GEMM.

    x [nimg, H, W, C1] (+ x2 [nimg, H, W, C2] concatenated on C); weight [Cout, ks, ks, C1+C2] contiguous
    (== a channels_last-format nn.Conv2d weight); returns [nimg, Ho, Wo, Cout].  `upsample`: x/x2 are at half
    resolution and are read as their nearest-2x upsampling.  rowvec [nvec, Cout] is added to rows
    [i*rows_per_vec, (i+1)*rows_per_vec) (time embedding); residual [nimg, Ho, Wo, Cout] is added last.
    `padding` = (before, after) zero rows/columns (default ks//2 each); (0, 1) is diffusers' Downsample2D(padding=0).
    """
    _chk(x, 'x'); _chk(x2, 'x2'); _chk(weight, 'weight'); _chk(bias, 'bias'); _chk(rowvec, 'rowvec')
    _chk(residual, 'residual')
    nimg, Hs, Ws, C1 = x.shape
    C2 = x2.shape[-1] if x2 is not None else 0
    Cout, ks = weight.shape[0], weight.shape[1]
    if weight.shape[2] != ks or weight.shape[3] != C1 + C2:
        raise _lib.VsxError(f'conv2d: weight {tuple(weight.shape)} does not match input channels {C1}+{C2}')
    H, W = (Hs * 2, Ws * 2) if upsample else (Hs, Ws)
    pad_lo, pad_hi = (ks // 2, ks // 2) if padding is None else padding      # (before, after) on both spatial axes
    Ho = (H + pad_lo + pad_hi - ks) // stride + 1
    Wo = (W + pad_lo + pad_hi - ks) // stride + 1
    out = torch.empty(nimg, Ho, Wo, Cout, dtype=_F16, device=x.device)
    d = GemmDesc()
    if padding is not None:
        d.pad_lo, d.pad_hi = pad_lo, pad_hi
    d.M, d.N, d.K = nimg * Ho * Wo, Cout, ks * ks * (C1 + C2)
    d.batch0 = d.batch1 = 1
    d.A = x.data_ptr(); d.A2 = x2.data_ptr() if x2 is not None else None
    d.a_mode = 1; d.H, d.W, d.C1, d.C2 = H, W, C1, C2
    d.ks, d.stride, d.upsample = ks, stride, 1 if upsample else 0
    d.B = weight.data_ptr(); d.ldb = d.K
    d.C = out.data_ptr(); d.ldc = Cout
    d.bias = bias.data_ptr() if bias is not None else None
    if rowvec is not None:
        d.rowvec = rowvec.data_ptr(); d.rows_per_vec = rows_per_vec
    if residual is not None:
        if residual.numel() != out.numel():
            raise _lib.VsxError('conv2d: residual shape mismatch')
        d.residual = residual.data_ptr(); d.ldr = Cout
    d.alpha = 1.0
    form = _conv_form(d)
    if form == 'subpixel':
        w4 = subpixel_weights(weight)
        d.B = w4.data_ptr()
        gemm(d, k_flop=4 * C1)
    elif form == 'winograd':
        _conv_winograd(d, weight, x.device)
    else:
        gemm(d)
    return out


def attention_scores(q, k, heads, scale, kv_div=1, causal=False, softmax=True):
    """probs = softmax(scale * q k^T) materialised (the Prompt-to-Prompt hook path).

    q [nb, nq, C], k [nkvb, nk, C] -> probs [nb, heads, nq, nk] (a view of a buffer whose rows are padded to a
    multiple of 8 so that probs @ V can stream it with 16-byte loads)."""
    _chk(q, 'q'); _chk(k, 'k')
    nb, nq, C = q.shape
    nk = k.shape[1]
    dh = C // heads
    ld = round_up(nk, 8)
    buf = torch.empty(nb, heads, nq, ld, dtype=_F16, device=q.device)
    if ld != nk:
        buf.zero_()
    if kv_div == 1:
        d = GemmDesc()
        d.M, d.N, d.K = nq, nk, dh
        d.batch0, d.batch1 = nb, heads
        d.A = q.data_ptr(); d.lda = C; d.a_bs0 = nq * C; d.a_bs1 = dh
        d.B = k.data_ptr(); d.ldb = C; d.b_bs0 = nk * C; d.b_bs1 = dh
        d.C = buf.data_ptr(); d.ldc = ld; d.c_bs0 = heads * nq * ld; d.c_bs1 = nq * ld
        d.alpha = float(scale)
        gemm(d)
    else:
        for kb in range(k.shape[0]):  # text K shared by kv_div consecutive images
            d = GemmDesc()
            d.M, d.N, d.K = nq, nk, dh
            d.batch0, d.batch1 = kv_div, heads
            sl = q[kb * kv_div:(kb + 1) * kv_div]
            d.A = sl.data_ptr(); d.lda = C; d.a_bs0 = nq * C; d.a_bs1 = dh
            d.B = k[kb].data_ptr(); d.ldb = C; d.b_bs0 = 0; d.b_bs1 = dh
            d.C = buf[kb * kv_div:(kb + 1) * kv_div].data_ptr(); d.ldc = ld
            d.c_bs0 = heads * nq * ld; d.c_bs1 = nq * ld
            d.alpha = float(scale)
            gemm(d)
    if not softmax:                  # the raw scaled products (gradient path: dP = dO V^T has the same shape)
        return buf[..., :nk]
    return softmax_rows(buf[..., :nk], rows_per_seq=nq if causal else None)


def softmax_rows(scores, rows_per_seq=None):
    """In-place softmax over the last axis of `scores` [.., nk]: a contiguous tensor or the view `buf[..., :nk]` of a buffer
    whose rows are padded to ld >= nk (the padding is not touched).  rows_per_seq: causal form, row r is query
    r % rows_per_seq and columns beyond it come out as exact zeros.  Returns `scores`."""
    _chk_view(scores, 'scores')
    nk = scores.shape[-1]
    ld = scores.stride(-2) if scores.dim() >= 2 else nk
    dense, step = True, ld                  # every leading axis continues the row sequence (axes of size 1 aside)
    for i in range(scores.dim() - 2, -1, -1):
        dense = dense and (scores.shape[i] == 1 or scores.stride(i) == step)
        step *= scores.shape[i]
    if scores.dim() < 2 or nk == 0 or scores.stride(-1) != 1 or ld < nk or not dense:
        raise _lib.VsxError(f'softmax_rows: need [.., nk] with unit inner stride and evenly spaced rows, got shape '
                            f'{tuple(scores.shape)} strides {scores.stride()}')
    nrows = scores.numel() // nk
    if rows_per_seq is None:
        check(_lib.load().vsx_softmax_rows(_p(scores), nrows, nk, ld, _stream()), 'vsx_softmax_rows')
    else:
        check(_lib.load().vsx_softmax_rows_causal(_p(scores), nrows, nk, ld, int(rows_per_seq), _stream()),
              'vsx_softmax_rows_causal')
    return scores


def head_scores(query, key, scale):
    """softmax(scale * q k^T) for head-batched operands [B*heads, N, d] x [B*heads, Nk, d] -> [B*heads, N, Nk]
    (diffusers `Attention.get_attention_scores`, the surface foreign processors call)."""
    query, key = query.contiguous(), key.contiguous()
    _chk(query, 'query'); _chk(key, 'key')
    nbh, nq, d = query.shape
    nk = key.shape[1]
    probs = torch.empty(nbh, nq, nk, dtype=_F16, device=query.device)
    g = GemmDesc()
    g.M, g.N, g.K = nq, nk, d
    g.batch0, g.batch1 = nbh, 1
    g.A = query.data_ptr(); g.lda = d; g.a_bs0 = nq * d
    g.B = key.data_ptr(); g.ldb = d; g.b_bs0 = nk * d
    g.C = probs.data_ptr(); g.ldc = nk; g.c_bs0 = nq * nk
    g.alpha = float(scale)
    gemm(g)
    return softmax_rows(probs)


def attention_pv(probs, vt, kv_div=1):
    """out[b, q, h*d + c] = sum_t probs[b, h, q, t] * vt[b // kv_div, h*d + c, t]; probs from attention_scores
    (possibly edited in place by a controller; must still be a view of a buffer with padded rows)."""
    nb, heads, nq, nk = probs.shape
    ld = probs.stride(2)
    if probs.stride(3) != 1 or probs.stride(1) != nq * ld or probs.stride(0) != heads * nq * ld or ld % 8:
        ld = round_up(nk, 8)
        buf = torch.zeros(nb, heads, nq, ld, dtype=_F16, device=probs.device)
        buf[..., :nk] = probs
        probs = buf[..., :nk]
    if probs.dtype != _F16 or not probs.is_cuda:
        raise _lib.VsxError('attention_pv: probs must be an fp16 GPU tensor')
    _chk(vt, 'vt')
    C, ldvt = vt.shape[1], vt.shape[2]
    dh = C // heads
    out = torch.empty(nb, nq, C, dtype=_F16, device=probs.device)
    # K (reduction) = nk rounded up to 8: padded columns of probs are zero, padded VT columns masked by them
    kred = round_up(nk, 8)
    if ldvt < kred:
        raise _lib.VsxError('attention_pv: vt rows are shorter than round_up(nk, 8)')
    groups = [(0, nb, 0)] if kv_div == 1 else [(kb * kv_div, kv_div, kb) for kb in range(vt.shape[0])]
    for (b0, cnt, kb) in groups:
        d = GemmDesc()
        d.M, d.N, d.K = nq, dh, kred
        d.batch0, d.batch1 = cnt, heads
        d.A = probs[b0:].data_ptr(); d.lda = ld; d.a_bs0 = heads * nq * ld; d.a_bs1 = nq * ld
        d.B = vt[kb if kv_div != 1 else b0:].data_ptr(); d.ldb = ldvt
        d.b_bs0 = 0 if kv_div != 1 else C * ldvt; d.b_bs1 = dh * ldvt
        d.C = out[b0:].data_ptr(); d.ldc = C; d.c_bs0 = nq * C; d.c_bs1 = dh
        d.alpha = 1.0
        gemm(d)
    return out


def _rows_view(t, name):
    """[n, rows, C] tensor or column-slice view of a wider [n, rows, W] buffer (fused q|k|v projections): returns
    (row stride, batch stride) in elements after checking what the kernels need."""
    _chk_view(t, name)
    if t.dim() != 3 or t.stride(2) != 1 or t.stride(1) % 8 or t.stride(0) % 8 or (t.data_ptr() % 16):
        raise _lib.VsxError(f'{name}: need unit inner stride, 16-byte aligned base, strides multiple of 8 (got {t.stride()})')
    return t.stride(1), t.stride(0)


def _chk_view(t, name):
    if not t.is_cuda or t.dtype != _F16:
        raise _lib.VsxError(f'{name}: expected an fp16 GPU tensor')


def attention(q, k, vt, heads, scale, kv_div=1, nk=None):
    """Fused softmax(q k^T * scale) v.  q [nb,nq,C]; k [nkvb,nk,C] (both may be column slices of a fused projection
    buffer); vt [nkvb,C,ldvt] -> [nb,nq,C]."""
    _chk(vt, 'vt')
    ldq, q_bs = _rows_view(q, 'q')
    ldk, k_bs = _rows_view(k, 'k')
    nb, nq, C = q.shape
    nk = k.shape[1] if nk is None else nk
    dh = C // heads
    out = torch.empty(nb, nq, C, dtype=_F16, device=q.device)
    if FlopCounter.enabled:
        FlopCounter.attention += 4.0 * nb * heads * nq * nk * dh
    check(_lib.load().vsx_attention_f16(_p(q), _p(k), _p(vt), _p(out), nb, heads, nq, nk, dh, ldq, ldk, vt.shape[2], C,
                                        q_bs, k_bs, C * vt.shape[2], nq * C, kv_div, float(scale),
                                        _stream()), 'vsx_attention_f16')
    return out


def temporal_attention(q, k, v, B, fq, fk, hw, heads, scale):
    """q [B*fq*hw, C], k/v [B*fk*hw, C] in (b, f, site) row order (possibly column slices of one fused q|k|v
    buffer) -> [B*fq*hw, C]."""
    for t, n in ((q, 'q'), (k, 'k'), (v, 'v')):
        _chk_view(t, n)
        if t.dim() != 2 or t.stride(1) != 1 or t.stride(0) % 8 or t.data_ptr() % 16:
            raise _lib.VsxError(f'{n}: need a [rows, C] tensor with unit inner stride and aligned rows')
    if k.stride(0) != v.stride(0):
        raise _lib.VsxError('temporal_attention: k and v must share their row stride')
    C = q.shape[-1]
    out = torch.empty(q.shape[0], C, dtype=_F16, device=q.device)
    if FlopCounter.enabled:
        FlopCounter.attention += 4.0 * B * hw * fq * fk * C
    fn = _lib.load().vsx_temporal_attention_f16
    if fq <= 32 or fk > 128:
        check(fn(_p(q), _p(k), _p(v), _p(out), B, fq, fk, hw, heads, C // heads, q.stride(0), k.stride(0), C,
                 float(scale), _stream()), 'vsx_temporal_attention_f16')
        return out
    # more than 32 query frames (a long clip whose frames are all local: FrameShard exchange='sites'): the matrix-core
    # kernel takes up to 32 query frames against up to 128 key frames, so the queries go in blocks of 32 frames; a
    # block's rows are contiguous within one batch item, hence one launch per (batch item, block)
    for b in range(B):
        kb, vb = k[b * fk * hw:(b + 1) * fk * hw], v[b * fk * hw:(b + 1) * fk * hw]
        for f0 in range(0, fq, 32):
            n = min(32, fq - f0)
            r0 = (b * fq + f0) * hw
            check(fn(_p(q[r0:r0 + n * hw]), _p(kb), _p(vb), _p(out[r0:r0 + n * hw]), 1, n, fk, hw, heads, C // heads,
                     q.stride(0), k.stride(0), C, float(scale), _stream()), 'vsx_temporal_attention_f16')
    return out


# --------------------------------------------------------------------------------------------
# normalisation
# --------------------------------------------------------------------------------------------
def group_norm(x, gamma, beta, groups, eps, nimg, silu=False, x2=None, partial_hook=None, count_rows=None):
    """GroupNorm over channels-last x (viewed as [nimg, rows, C1]) (+x2 concatenated on C) -> [.., C1+C2].

    nimg = B reproduces the reference's 5-D GroupNorm (statistics over all frames), nimg = B*F the per-frame one.
    partial_hook(partial) may all-reduce the fp32 partial sums in frame-sharded mode (count_rows = global rows).
    """
    _chk(x, 'x'); _chk(x2, 'x2'); _chk(gamma, 'gamma'); _chk(beta, 'beta')
    C1 = x.shape[-1]
    C2 = x2.shape[-1] if x2 is not None else 0
    rows = x.numel() // C1 // nimg
    lib = _lib.load()
    nchunks = lib.vsx_groupnorm_chunks(rows, nimg)
    partial = torch.empty(nimg, nchunks, groups, 2, dtype=torch.float32, device=x.device)
    s = _stream()
    check(lib.vsx_groupnorm_stats(_p(x), _p(x2), nimg, rows, C1, C2, groups, _p(partial), s), 'vsx_groupnorm_stats')
    if partial_hook is not None:
        partial = partial_hook(partial)
        nchunks = partial.shape[1]
    y = torch.empty(*x.shape[:-1], C1 + C2, dtype=_F16, device=x.device)
    stats = torch.empty(nimg, groups, 2, dtype=torch.float32, device=x.device)
    check(lib.vsx_groupnorm_apply(_p(x), _p(x2), nimg, rows, C1, C2, groups, _p(partial), nchunks,
                                  rows if count_rows is None else count_rows, _p(gamma), _p(beta), float(eps),
                                  1 if silu else 0, _p(stats), _p(y), s), 'vsx_groupnorm_apply')
    return y


def layer_norm(x, gamma, beta, eps=1e-5, pe=None, rows_per_frame=0, frames=0, frame_offset=0):
    if isinstance(x, DeferredLN):
        raise _lib.VsxError('layer_norm of a deferred LayerNorm: materialize() it first')
    _chk(x, 'x'); _chk(gamma, 'gamma'); _chk(beta, 'beta'); _chk(pe, 'pe')
    C = x.shape[-1]
    if pe is not None:
        # the kernel indexes pe[(row / rows_per_frame) % frames + frame_offset]: a clip longer than the table
        # (temporal_position_encoding_max_len) must fail like the reference's shape error, not read past the table
        if pe.dim() != 2 or pe.shape[1] != C or frames <= 0 or rows_per_frame <= 0 or frame_offset < 0 \
                or pe.shape[0] < frame_offset + frames:
            raise _lib.VsxError(f'layer_norm: positional-encoding table {tuple(pe.shape)} does not cover frames '
                                f'[{frame_offset}, {frame_offset + frames}) x {C} channels')
    y = torch.empty_like(x)
    check(_lib.load().vsx_layernorm(_p(x), x.numel() // C, C, _p(gamma), _p(beta), float(eps), _p(pe), rows_per_frame,
                                    frames, frame_offset, _p(y), _stream()), 'vsx_layernorm')
    return y


# --------------------------------------------------------------------------------------------
# element-wise glue
# --------------------------------------------------------------------------------------------
def silu(x):
    _chk(x, 'x')
    y = torch.empty_like(x)
    check(_lib.load().vsx_silu(_p(x), _p(y), x.numel(), _stream()), 'vsx_silu')
    return y


def quick_gelu(x):
    _chk(x, 'x')
    y = torch.empty_like(x)
    check(_lib.load().vsx_quick_gelu(_p(x), _p(y), x.numel(), _stream()), 'vsx_quick_gelu')
    return y


def axpy(a, b, s=1.0):
    _chk(a, 'a'); _chk(b, 'b')
    if a.shape != b.shape:
        raise _lib.VsxError(f'axpy: shape mismatch {tuple(a.shape)} vs {tuple(b.shape)}')
    y = torch.empty_like(a)
    check(_lib.load().vsx_axpy(_p(a), _p(b), float(s), _p(y), a.numel(), _stream()), 'vsx_axpy')
    return y


def pack_latents(x, cpad=8):
    """[B,C,F,H,W] -> channels-last [B*F,H,W,cpad] (zero-padded channels)."""
    _chk(x, 'x')
    B, C, F, H, W = x.shape
    y = torch.empty(B * F, H, W, cpad, dtype=_F16, device=x.device)
    check(_lib.load().vsx_pack_latents(_p(x), _p(y), B, C, F, H * W, cpad, _stream()), 'vsx_pack_latents')
    return y


def unpack_latents(x, B, cout):
    """channels-last [B*F,H,W,Cs] -> [B,cout,F,H,W]."""
    _chk(x, 'x')
    BF, H, W, Cs = x.shape
    F = BF // B
    y = torch.empty(B, cout, F, H, W, dtype=_F16, device=x.device)
    check(_lib.load().vsx_unpack_latents(_p(x), _p(y), B, cout, F, H * W, Cs, _stream()), 'vsx_unpack_latents')
    return y


def cfg_ddim_step(x, eps_u, eps_c, guidance, alpha_t, alpha_next):
    _chk(x, 'x'); _chk(eps_u, 'eps_u'); _chk(eps_c, 'eps_c')
    out = torch.empty_like(x)
    check(_lib.load().vsx_cfg_ddim_step(_p(x), _p(eps_u), _p(eps_c), float(guidance), float(alpha_t),
                                        float(alpha_next), _p(out), x.numel(), _stream()), 'vsx_cfg_ddim_step')
    return out


def masked_blend(x, src, mask):
    """x, src [C, ...spatial]; mask [...spatial] -> src + mask*(x-src)."""
    _chk(x, 'x'); _chk(src, 'src'); _chk(mask, 'mask')
    C = x.shape[0]
    n_sp = x.numel() // C
    if mask.numel() != n_sp or src.shape != x.shape:
        raise _lib.VsxError('masked_blend: shape mismatch')
    out = torch.empty_like(x)
    check(_lib.load().vsx_masked_blend(_p(x), _p(src), _p(mask), _p(out), C, n_sp, _stream()), 'vsx_masked_blend')
    return out


def adapter_scatter(tracks, selected, feat, h, w, rate, out_scale=1.0):
    """tracks [F,P,2] fp32, selected [P] int32, feat [P,C] fp16 -> [F,h,w,C] fp16."""
    _chk(tracks, 'tracks', torch.float32); _chk(selected, 'selected', torch.int32); _chk(feat, 'feat')
    F, P = tracks.shape[:2]
    C = feat.shape[1]
    out = torch.zeros(F, h, w, C, dtype=_F16, device=feat.device)
    check(_lib.load().vsx_adapter_scatter(_p(tracks), _p(selected), _p(feat), _p(out), F, P, C, h, w, float(rate),
                                          float(out_scale), _stream()), 'vsx_adapter_scatter')
    return out


def _dift_feat(feat):
    _chk(feat, 'feat')
    if feat.dim() != 5 or feat.shape[-1] % 8:
        raise _lib.VsxError(f'dift: feat must be [N, E, h, w, C] with C % 8 == 0, got {tuple(feat.shape)}')
    return feat.shape


def _dift_query(query, N, lead, C, name='query'):
    """[lead, C] (shared by all frames) or [N, lead, C] fp32 -> per-frame flag"""
    _chk(query, name, torch.float32)
    if query.shape[-1] != C or tuple(query.shape[:-1]) not in ((lead,), (N, lead)):
        raise _lib.VsxError(f'dift: {name} must be [{lead}, {C}] or [{N}, {lead}, {C}], got {tuple(query.shape)}')
    return int(query.dim() == 3)


def dift_sample_points(feat, size, coords, query=None, want_cos=False):
    """feat fp16 [N, E, h, w, C] (the UNet tap, ensemble members of a frame adjacent); size (H, W) of the image;
    coords int32 [N, P, 2] = pixel (x, y), x < 0 = skip -> (vec fp32 [N, P, C], cos fp32 [N, P] or None).  vec is the
    bilinear (align_corners=False) upsampling of the ensemble mean to (H, W), read at (y, x)."""
    N, E, h, w, C = _dift_feat(feat)
    _chk(coords, 'coords', torch.int32)
    if coords.dim() != 3 or coords.shape[0] != N or coords.shape[2] != 2:
        raise _lib.VsxError(f'dift_sample_points: coords must be [{N}, P, 2], got {tuple(coords.shape)}')
    P = coords.shape[1]
    H, W = (int(s) for s in size)
    per_frame = 0
    if query is not None:
        per_frame = _dift_query(query, N, P, C)
    elif want_cos:
        raise _lib.VsxError('dift_sample_points: cos needs query vectors')
    vec = torch.empty(N, P, C, dtype=torch.float32, device=feat.device)
    cos = torch.empty(N, P, dtype=torch.float32, device=feat.device) if want_cos else None
    check(_lib.load().vsx_dift_sample_points(_p(feat), N, E, h, w, C, H, W, _p(coords), P, _p(query), per_frame,
                                             _p(vec), _p(cos), _stream()), 'vsx_dift_sample_points')
    return vec, cos


def dift_cosine_map(feat, size, query, want_map=True):
    """feat fp16 [N, E, h, w, C]; query fp32 [Q, C] or [N, Q, C] -> (cos map fp32 [N, Q, H, W] or None,
    argmax int32 [N, Q, 2] = (y, x) (first in row-major order among equal values), max fp32 [N, Q]).  Never builds the
    upsampled [C, H, W] map (csrc/dift.hip)."""
    N, E, h, w, C = _dift_feat(feat)
    Q = query.shape[-2]
    per_frame = _dift_query(query, N, Q, C)
    H, W = (int(s) for s in size)
    lib = _lib.load()
    ws = torch.empty(lib.vsx_dift_cosine_map_workspace(N, h, w, C, Q), dtype=torch.uint8, device=feat.device)
    cmap = torch.empty(N, Q, H, W, dtype=torch.float32, device=feat.device) if want_map else None
    yx = torch.empty(N, Q, 2, dtype=torch.int32, device=feat.device)
    val = torch.empty(N, Q, dtype=torch.float32, device=feat.device)
    check(lib.vsx_dift_cosine_map(_p(feat), N, E, h, w, C, H, W, _p(query), Q, per_frame, _p(ws), ws.numel(), _p(cmap),
                                  _p(yx), _p(val), _stream()), 'vsx_dift_cosine_map')
    return cmap, yx, val


_COORD_PE = {'none': 0, 'encoding': 1, 'hash_encoding': 2}
_COORD_MLP = {'origin': 0, 'tcnn': 1}


def _skip_mask(skip_layers, what):
    """skip_layers -> the bit mask the entry points take (bit i: layer i sees the encoded input again)"""
    mask = 0
    for i in skip_layers:
        if not 0 <= int(i) < 62:
            raise NotImplementedError(f'{what}: skip_layers {list(skip_layers)}')
        mask |= 1 << int(i)
    return mask


def _check_supported(rc, what):
    """`check`, with VSX_E_UNSUPPORTED (an option the kernel does not implement) as NotImplementedError"""
    if rc == _lib.VSX_E_UNSUPPORTED:
        raise NotImplementedError(_lib.load().vsx_last_error().decode(errors='replace'))
    check(rc, what)


def coord_mlp(x, packed, input_dim, output_dim, hidden_dim, mlp_layers, pe_type='none', pe_dim=0, mlp_type='origin',
              skip_layers=(), use_tanh=True):
    """The whole network of IMLP_Hash.forward (mlp_type 'origin') in one launch, fp32 throughout: x fp32 [N, input_dim]
    -> fp32 [N, output_dim].  `packed`: the weights and biases in the kernel's layout (atlas.pack_coord_mlp; vsx.h K13).
    Options the kernel does not implement raise NotImplementedError."""
    if pe_type not in _COORD_PE:
        raise NotImplementedError(f'coord_mlp: pe_type {pe_type!r} (IMLP_Hash knows none / encoding / hash_encoding)')
    if mlp_type not in _COORD_MLP:
        raise NotImplementedError(f'coord_mlp: mlp_type {mlp_type!r} (IMLP_Hash knows origin / tcnn)')
    _chk(x, 'x', torch.float32)
    _chk(packed, 'packed', torch.float32)
    if x.dim() != 2 or x.shape[1] != input_dim:
        raise _lib.VsxError(f'coord_mlp: x must be [N, {input_dim}], got {tuple(x.shape)}')
    mask = _skip_mask(skip_layers, 'coord_mlp')
    out = torch.empty(x.shape[0], int(output_dim), dtype=torch.float32, device=x.device)
    lib = _lib.load()
    rc = lib.vsx_coord_mlp_f32(_p(x), x.shape[0], int(input_dim), int(output_dim), int(hidden_dim), int(mlp_layers),
                               _COORD_PE[pe_type], int(pe_dim), _COORD_MLP[mlp_type], mask, int(bool(use_tanh)),
                               _p(packed), packed.numel(), _p(out), _stream())
    _check_supported(rc, 'vsx_coord_mlp_f32')
    return out


COORD_MLP_WGRAD_ROWS = 512     # vsx_coord_mlp_wgrad_rows(): rows per chunk of the weight-gradient reduction (csrc/atlas_bwd.hip)


def _coord_net(what, input_dim, output_dim, hidden_dim, mlp_layers, pe_type, pe_dim, mlp_type, skip_layers):
    """the nine integers by which the K13 / K16 entry points know a network"""
    if pe_type not in _COORD_PE:
        raise NotImplementedError(f'{what}: pe_type {pe_type!r} (IMLP_Hash knows none / encoding / hash_encoding)')
    if mlp_type not in _COORD_MLP:
        raise NotImplementedError(f'{what}: mlp_type {mlp_type!r} (IMLP_Hash knows origin / tcnn)')
    return (int(input_dim), int(output_dim), int(hidden_dim), int(mlp_layers), _COORD_PE[pe_type], int(pe_dim),
            _COORD_MLP[mlp_type], _skip_mask(skip_layers, what))


def coord_mlp_train_workspace(N, input_dim, output_dim, hidden_dim, mlp_layers, pe_type='none', pe_dim=0, mlp_type='origin',
                              skip_layers=()):
    """-> (saved, scratch, grad): the float counts of the three buffers of a training step over N rows (vsx.h K16)"""
    net = _coord_net('coord_mlp_train_workspace', input_dim, output_dim, hidden_dim, mlp_layers, pe_type, pe_dim, mlp_type,
                     skip_layers)
    counts = [ctypes.c_int64(0) for _ in range(3)]
    rc = _lib.load().vsx_coord_mlp_train_workspace(int(N), *net, *(ctypes.addressof(c) for c in counts))
    _check_supported(rc, 'vsx_coord_mlp_train_workspace')
    return tuple(int(c.value) for c in counts)


def coord_mlp_train_forward(x, packed, input_dim, output_dim, hidden_dim, mlp_layers, pe_type='none', pe_dim=0,
                            mlp_type='origin', skip_layers=(), use_tanh=True, saved=None):
    """`coord_mlp` (the same kernel source, the same bits) that also stores what `coord_mlp_backward` reads -> (out, saved):
    saved fp32, flat (vsx.h K16: the hidden activations after their ReLU, the encoded input, out).  `saved`: a buffer to
    fill instead of a new one; one shorter than `coord_mlp_train_workspace` says is refused (VsxError)."""
    net = _coord_net('coord_mlp_train_forward', input_dim, output_dim, hidden_dim, mlp_layers, pe_type, pe_dim, mlp_type, skip_layers)
    _chk(x, 'x', torch.float32)
    _chk(packed, 'packed', torch.float32)
    _chk(saved, 'saved', torch.float32)
    if x.dim() != 2 or x.shape[1] != input_dim:
        raise _lib.VsxError(f'coord_mlp_train_forward: x must be [N, {input_dim}], got {tuple(x.shape)}')
    lib = _lib.load()
    if saved is None:
        floats = ctypes.c_int64(0)
        _check_supported(lib.vsx_coord_mlp_train_workspace(x.shape[0], *net, ctypes.addressof(floats), None, None),
                         'vsx_coord_mlp_train_workspace')
        saved = torch.empty(floats.value, dtype=torch.float32, device=x.device)
    out = torch.empty(x.shape[0], int(output_dim), dtype=torch.float32, device=x.device)
    rc = lib.vsx_coord_mlp_fwd_train_f32(_p(x), x.shape[0], *net, int(bool(use_tanh)), _p(packed), packed.numel(), _p(out),
                                         _p(saved), saved.numel(), _stream())
    _check_supported(rc, 'vsx_coord_mlp_fwd_train_f32')
    return out, saved


def coord_mlp_backward(grad_out, saved, packed, input_dim, output_dim, hidden_dim, mlp_layers, pe_type='none', pe_dim=0,
                       mlp_type='origin', skip_layers=(), use_tanh=True, grad=None):
    """Weight and bias gradients of the network `coord_mlp_train_forward` ran: grad_out fp32 [N, output_dim], `saved` and
    `packed` of that call -> one flat fp32 buffer: per layer the weight gradient [out, in] (nn.Linear layout, unpadded),
    then the bias gradient.  No gradient with respect to x.  Deterministic: no atomics, a fixed summation order.  `grad`:
    a buffer to fill instead of a new one; a short `saved` or `grad` is refused (VsxError)."""
    net = _coord_net('coord_mlp_backward', input_dim, output_dim, hidden_dim, mlp_layers, pe_type, pe_dim, mlp_type, skip_layers)
    _chk(grad_out, 'grad_out', torch.float32)
    _chk(saved, 'saved', torch.float32)
    _chk(packed, 'packed', torch.float32)
    _chk(grad, 'grad', torch.float32)
    if grad_out.dim() != 2 or grad_out.shape[1] != output_dim:
        raise _lib.VsxError(f'coord_mlp_backward: grad_out must be [N, {output_dim}], got {tuple(grad_out.shape)}')
    lib = _lib.load()
    N = grad_out.shape[0]
    counts = [ctypes.c_int64(0) for _ in range(2)]
    _check_supported(lib.vsx_coord_mlp_train_workspace(N, *net, None, *(ctypes.addressof(c) for c in counts)),
                     'vsx_coord_mlp_train_workspace')
    scratch = torch.empty(counts[0].value, dtype=torch.float32, device=grad_out.device)
    if grad is None:
        grad = torch.empty(counts[1].value, dtype=torch.float32, device=grad_out.device)
    rc = lib.vsx_coord_mlp_bwd_f32(_p(grad_out), N, *net, int(bool(use_tanh)), _p(packed), packed.numel(), _p(saved), saved.numel(),
                                   _p(scratch), scratch.numel(), _p(grad), grad.numel(), _stream())
    _check_supported(rc, 'vsx_coord_mlp_bwd_f32')
    return grad


def _hash_grid_args(x, table, grid, what):
    """(input_dim, table_floats, n_levels, n_features, log2_hashmap_size, base_resolution, per_level_scale) of a call"""
    _chk(x, 'x', torch.float32)
    _chk(table, 'table', torch.float32)
    if x.dim() != 2 or table.dim() != 1:
        raise _lib.VsxError(f'{what}: x must be [N, input_dim] and the table flat, got {tuple(x.shape)} / {tuple(table.shape)}')
    return (x.shape[1], _p(table), table.numel(), int(grid['n_levels']), int(grid['n_features_per_level']),
            int(grid['log2_hashmap_size']), int(grid['base_resolution']), float(grid['per_level_scale']))


def hash_grid(x, table, grid):
    """tiny-cuda-nn's HashGrid (Linear interpolation) as include/vsx.h K14 restates it: x fp32 [N, 2], table fp32 (flat,
    level-major), grid = the encoding_config dict -> fp32 [N, n_levels * n_features_per_level].  Configurations the kernel
    does not implement raise NotImplementedError."""
    d, tab, floats, *cfg = _hash_grid_args(x, table, grid, 'hash_grid')
    out = torch.empty(x.shape[0], cfg[0] * cfg[1], dtype=torch.float32, device=x.device)
    lib = _lib.load()
    rc = lib.vsx_hash_grid_f32(_p(x), x.shape[0], d, tab, floats, *cfg, _p(out), _stream())
    _check_supported(rc, 'vsx_hash_grid_f32')
    return out


def hash_mlp(x, table, grid, packed, output_dim, hidden_dim, mlp_layers, skip_layers=(), use_tanh=True):
    """IMLP_Hash.forward with pe_type 'hash_encoding', mlp_type 'origin' in one launch: `hash_grid` feeding the layer stack
    of `coord_mlp` (`packed`: atlas.pack_coord_mlp with n_levels * n_features_per_level encoded columns).  x fp32 [N, 2]
    -> fp32 [N, output_dim]."""
    d, tab, floats, *cfg = _hash_grid_args(x, table, grid, 'hash_mlp')
    _chk(packed, 'packed', torch.float32)
    mask = _skip_mask(skip_layers, 'hash_mlp')
    out = torch.empty(x.shape[0], int(output_dim), dtype=torch.float32, device=x.device)
    lib = _lib.load()
    rc = lib.vsx_hash_mlp_f32(_p(x), x.shape[0], d, tab, floats, *cfg, int(output_dim), int(hidden_dim), int(mlp_layers),
                              mask, int(bool(use_tanh)), _p(packed), packed.numel(), _p(out), _stream())
    _check_supported(rc, 'vsx_hash_mlp_f32')
    return out


def _hash_net(output_dim, hidden_dim, mlp_layers, skip_layers, what):
    return int(output_dim), int(hidden_dim), int(mlp_layers), _skip_mask(skip_layers, what)


def hash_grid_backward(x, grad_enc, table, grid, want_table=True, want_x=True):
    """The gradients of `hash_grid` alone (include/vsx.h K17): x fp32 [N, 2], grad_enc fp32 [N, n_levels *
    n_features_per_level] -> (grad_table, grad_x): fp32 flat like `table` / fp32 [N, 2]; None where not wanted.  grad_x is
    deterministic; grad_table is a scatter-add with fp32 atomics and is NOT bit-reproducible from run to run."""
    d, tab, floats, *cfg = _hash_grid_args(x, table, grid, 'hash_grid_backward')
    _chk(grad_enc, 'grad_enc', torch.float32)
    if grad_enc.dim() != 2 or tuple(grad_enc.shape) != (x.shape[0], cfg[0] * cfg[1]):
        raise _lib.VsxError(f'hash_grid_backward: grad_enc must be [{x.shape[0]}, {cfg[0] * cfg[1]}], got {tuple(grad_enc.shape)}')
    grad_table = torch.empty_like(table) if want_table else None
    grad_x = torch.empty_like(x) if want_x else None
    rc = _lib.load().vsx_hash_grid_bwd_f32(_p(x), x.shape[0], d, _p(grad_enc), tab, floats, *cfg, _p(grad_table), _p(grad_x),
                                           _stream())
    _check_supported(rc, 'vsx_hash_grid_bwd_f32')
    return grad_table, grad_x


def hash_mlp_train_workspace(N, grid, output_dim, hidden_dim, mlp_layers, skip_layers=(), input_dim=2):
    """-> (saved, scratch, grad): the float counts of the three buffers of a training step of `hash_mlp` over N rows
    (vsx.h K17; grad covers the layers only)"""
    counts = [ctypes.c_int64(0) for _ in range(3)]
    rc = _lib.load().vsx_hash_mlp_train_workspace(
        int(N), int(input_dim), int(grid['n_levels']), int(grid['n_features_per_level']), int(grid['log2_hashmap_size']),
        int(grid['base_resolution']), float(grid['per_level_scale']),
        *_hash_net(output_dim, hidden_dim, mlp_layers, skip_layers, 'hash_mlp_train_workspace'),
        *(ctypes.addressof(c) for c in counts))
    _check_supported(rc, 'vsx_hash_mlp_train_workspace')
    return tuple(int(c.value) for c in counts)


def hash_mlp_train_forward(x, table, grid, packed, output_dim, hidden_dim, mlp_layers, skip_layers=(), use_tanh=True, saved=None):
    """`hash_mlp` (the same kernel source, the same bits) that also stores what `hash_mlp_backward` reads -> (out, saved):
    saved fp32, flat (vsx.h K17: the hidden activations after their ReLU, the grid's features, out).  `saved`: a buffer to
    fill instead of a new one; one shorter than `hash_mlp_train_workspace` says is refused (VsxError)."""
    d, tab, floats, *cfg = _hash_grid_args(x, table, grid, 'hash_mlp_train_forward')
    _chk(packed, 'packed', torch.float32)
    _chk(saved, 'saved', torch.float32)
    net = _hash_net(output_dim, hidden_dim, mlp_layers, skip_layers, 'hash_mlp_train_forward')
    lib = _lib.load()
    if saved is None:
        n_saved = ctypes.c_int64(0)
        _check_supported(lib.vsx_hash_mlp_train_workspace(x.shape[0], d, *cfg, *net, ctypes.addressof(n_saved), None, None),
                         'vsx_hash_mlp_train_workspace')
        saved = torch.empty(n_saved.value, dtype=torch.float32, device=x.device)
    out = torch.empty(x.shape[0], int(output_dim), dtype=torch.float32, device=x.device)
    rc = lib.vsx_hash_mlp_fwd_train_f32(_p(x), x.shape[0], d, tab, floats, *cfg, *net, int(bool(use_tanh)), _p(packed),
                                        packed.numel(), _p(out), _p(saved), saved.numel(), _stream())
    _check_supported(rc, 'vsx_hash_mlp_fwd_train_f32')
    return out, saved


def hash_mlp_backward(grad_out, x, table, grid, saved, packed, output_dim, hidden_dim, mlp_layers, skip_layers=(), use_tanh=True,
                      want_table=True, want_x=True, grad=None, scratch=None):
    """The gradients of the network `hash_mlp_train_forward` ran: grad_out fp32 [N, output_dim]; x, table, `saved` and
    `packed` of that call -> (grad, grad_table, grad_x): grad one flat fp32 buffer, per layer the weight gradient [out, in]
    (nn.Linear layout, unpadded), then the bias gradient; grad_table flat like `table`; grad_x [N, 2]; the last two None
    where not wanted.  grad and grad_x are deterministic (no atomics, fixed summation orders); grad_table is a scatter-add
    with fp32 atomics and is NOT bit-reproducible from run to run (vsx.h K17).  `grad` / `scratch`: buffers to use instead
    of new ones; a short `saved`, `scratch` or `grad` is refused (VsxError)."""
    d, tab, floats, *cfg = _hash_grid_args(x, table, grid, 'hash_mlp_backward')
    _chk(grad_out, 'grad_out', torch.float32)
    _chk(saved, 'saved', torch.float32)
    _chk(packed, 'packed', torch.float32)
    _chk(grad, 'grad', torch.float32)
    _chk(scratch, 'scratch', torch.float32)
    N = x.shape[0]
    if grad_out.dim() != 2 or tuple(grad_out.shape) != (N, int(output_dim)):
        raise _lib.VsxError(f'hash_mlp_backward: grad_out must be [{N}, {output_dim}], got {tuple(grad_out.shape)}')
    net = _hash_net(output_dim, hidden_dim, mlp_layers, skip_layers, 'hash_mlp_backward')
    lib = _lib.load()
    counts = [ctypes.c_int64(0) for _ in range(2)]
    _check_supported(lib.vsx_hash_mlp_train_workspace(N, d, *cfg, *net, None, *(ctypes.addressof(c) for c in counts)),
                     'vsx_hash_mlp_train_workspace')
    if scratch is None:
        scratch = torch.empty(counts[0].value, dtype=torch.float32, device=x.device)
    if grad is None:
        grad = torch.empty(counts[1].value, dtype=torch.float32, device=x.device)
    grad_table = torch.empty_like(table) if want_table else None
    grad_x = torch.empty_like(x) if want_x else None
    rc = lib.vsx_hash_mlp_bwd_f32(_p(grad_out), _p(x), N, d, tab, floats, *cfg, *net, int(bool(use_tanh)), _p(packed),
                                  packed.numel(), _p(saved), saved.numel(), _p(scratch), scratch.numel(), _p(grad), grad.numel(),
                                  _p(grad_table), _p(grad_x), _stream())
    _check_supported(rc, 'vsx_hash_mlp_bwd_f32')
    return grad, grad_table, grad_x


def atlas_edit(uv_fg, uv_bg, alpha, tex_fg, box_fg, tex_bg, box_bg, base_fg=None, base_bg=None, masks=None):
    """The texture-reading half of evaluate_model in one launch (include/vsx.h K15): uv_fg, uv_bg fp32 [N, 2] (the mapping
    networks' outputs), alpha fp32 [N] (0.001 .. 0.991), a texture fp32 [R, R, 3 or 4] and its box (minx, miny, pixel_size:
    atlas.texture_box) per layer -> (edit [N, 3], fg [N, 3], bg [N, 3], relevant uint8 [N]: bit 0 foreground, bit 1
    background).  A 4-channel texture is an RGBA overlay over base_fg / base_bg [N, 3].  masks = (mask_fg, mask_bg), fp32
    [R, R] each or None: updated in place (max with alpha / set to 1 where a relevant row lands).  Channel counts the
    kernel does not implement raise NotImplementedError, bad buffers VsxError."""
    _chk(uv_fg, 'uv_fg', torch.float32); _chk(uv_bg, 'uv_bg', torch.float32); _chk(alpha, 'alpha', torch.float32)
    _chk(tex_fg, 'tex_fg', torch.float32); _chk(tex_bg, 'tex_bg', torch.float32)
    _chk(base_fg, 'base_fg', torch.float32); _chk(base_bg, 'base_bg', torch.float32)
    mask_fg, mask_bg = (None, None) if masks is None else masks
    _chk(mask_fg, 'mask_fg', torch.float32); _chk(mask_bg, 'mask_bg', torch.float32)
    N = uv_fg.shape[0]
    if uv_fg.dim() != 2 or uv_fg.shape[1] != 2 or uv_bg.shape != uv_fg.shape or alpha.numel() != N:
        raise _lib.VsxError(f'atlas_edit: uv_fg / uv_bg must be [N, 2] and alpha [N], got {tuple(uv_fg.shape)} / '
                            f'{tuple(uv_bg.shape)} / {tuple(alpha.shape)}')
    layers = []
    for name, tex, box, base, mask in (('fg', tex_fg, box_fg, base_fg, mask_fg), ('bg', tex_bg, box_bg, base_bg, mask_bg)):
        if tex.dim() != 3:
            raise _lib.VsxError(f'atlas_edit: tex_{name} must be [R, R, C], got {tuple(tex.shape)}')
        if base is not None and tuple(base.shape) != (N, 3):
            raise _lib.VsxError(f'atlas_edit: base_{name} must be [{N}, 3], got {tuple(base.shape)}')
        if mask is not None and mask.dim() != 2:
            raise _lib.VsxError(f'atlas_edit: mask_{name} must be [R, R], got {tuple(mask.shape)}')
        minx, miny, pixel_size = (float(v) for v in box)
        layers += [_p(tex), tex.shape[0], tex.shape[1], tex.shape[2], minx, miny, pixel_size, _p(base), _p(mask),
                   mask.shape[0] if mask is not None else 0, mask.shape[1] if mask is not None else 0]
    edit, fg, bg = (torch.empty(N, 3, dtype=torch.float32, device=uv_fg.device) for _ in range(3))
    relevant = torch.empty(N, dtype=torch.uint8, device=uv_fg.device)
    lib = _lib.load()
    rc = lib.vsx_atlas_edit_f32(_p(uv_fg), _p(uv_bg), _p(alpha), N, *layers, _p(edit), _p(fg), _p(bg), _p(relevant), _stream())
    _check_supported(rc, 'vsx_atlas_edit_f32')
    return edit, fg, bg, relevant


ATLAS_DATA_KEYS = ('video_frames', 'video_frames_dx', 'video_frames_dy', 'mask_frames', 'optical_flows', 'optical_flows_reverse',
                   'optical_flows_mask', 'optical_flows_reverse_mask')
ATLAS_LOSSES = ('gradient_loss', 'rgb_loss', 'alpha_loss', 'sparsity_loss', 'rigidity_loss_fg', 'rigidity_loss_bg',
                'global_rigidity_loss_fg', 'global_rigidity_loss_bg', 'flow_loss_fg', 'flow_loss_bg', 'flow_alpha_loss', 'total_loss',
                'alpha_mean_fg', 'alpha_mean_bg')           # the order of `losses` (vsx.h K18)


def atlas_batch(idx, data, derivative_amount, global_derivative_amount, with_global_rigidity=True):
    """The data gather of an atlas training step in one launch (include/vsx.h K18a): idx int64 [N] or [N, 1], flat pixel
    indices in the (frame, row, column) order of get_tuples, on the CPU (checked against T H W there, then copied: 8 N bytes)
    or on the GPU (unchecked: the kernel gives such a row NaNs); `data`: load_input_data's data_dict on the GPU, fp32, in
    the reference's layouts -> dict(rows [B, N, 3] with B = 9 or 7, rgb / rgb_dx / rgb_dy [N, 3], alpha_gt / m_fwd / m_bwd
    [N], counts int32 [2], larger_dim, with_global_rigidity).  Every float is bit-equal to the reference's torch statement
    on the CPU.  Another flow level count than 1 raises NotImplementedError, bad buffers VsxError."""
    for k in ATLAS_DATA_KEYS:
        _chk(data[k], k, torch.float32)
    video, flows = data['video_frames'], data['optical_flows']
    if video.dim() != 4 or video.shape[2] != 3:
        raise _lib.VsxError(f'atlas_batch: video_frames must be [H, W, 3, T], got {tuple(video.shape)}')
    H, W, _, T = video.shape
    if flows.dim() != 5 or tuple(flows.shape[:4]) != (H, W, 2, T):
        raise _lib.VsxError(f'atlas_batch: optical_flows must be [{H}, {W}, 2, {T}, levels], got {tuple(flows.shape)}')
    levels = flows.shape[4]
    want = {'video_frames_dx': (H, W, 3, T), 'video_frames_dy': (H, W, 3, T), 'mask_frames': (H, W, T),
            'optical_flows_reverse': (H, W, 2, T, levels), 'optical_flows_mask': (H, W, T, levels),
            'optical_flows_reverse_mask': (H, W, T, levels)}
    for k, shape in want.items():
        if tuple(data[k].shape) != shape:
            raise _lib.VsxError(f'atlas_batch: {k} must be {list(shape)}, got {tuple(data[k].shape)}')
    idx = idx.reshape(-1)
    if idx.dtype != torch.int64:
        raise _lib.VsxError(f'atlas_batch: idx must be int64, got {idx.dtype}')
    N, dev = idx.numel(), video.device
    if not idx.is_cuda:
        if N and (int(idx.min()) < 0 or int(idx.max()) >= T * H * W):
            raise _lib.VsxError(f'atlas_batch: idx outside 0 .. {T * H * W - 1} (T H W = {T} x {H} x {W})')
        idx = idx.to(dev)
    idx = idx.contiguous()
    B = 9 if with_global_rigidity else 7
    f32 = dict(dtype=torch.float32, device=dev)
    out = dict(rows=torch.empty(B, N, 3, **f32), rgb=torch.empty(N, 3, **f32), rgb_dx=torch.empty(N, 3, **f32),
               rgb_dy=torch.empty(N, 3, **f32), alpha_gt=torch.empty(N, **f32), m_fwd=torch.empty(N, **f32),
               m_bwd=torch.empty(N, **f32), counts=torch.empty(2, dtype=torch.int32, device=dev))
    rc = _lib.load().vsx_atlas_batch_f32(
        _p(idx), N, H, W, T, levels, *(_p(data[k]) for k in ATLAS_DATA_KEYS), int(derivative_amount), int(global_derivative_amount),
        int(bool(with_global_rigidity)), *(_p(out[k]) for k in ('rows', 'rgb', 'rgb_dx', 'rgb_dy', 'alpha_gt', 'm_fwd', 'm_bwd', 'counts')),
        _stream())
    _check_supported(rc, 'vsx_atlas_batch_f32')
    out.update(larger_dim=max(H, W), with_global_rigidity=bool(with_global_rigidity))
    return out


def atlas_losses(uv_fg, uv_bg, alpha_raw, rgb_atlas, batch, cfg):
    """Every loss of an atlas training step and the gradient of total_loss with respect to the four network outputs, in
    two launches (include/vsx.h K18b): uv_fg, uv_bg fp32 [B N, 2] (the mapping networks on batch['rows']), alpha_raw [5 N]
    or [5 N, 1] (F_Alpha's tanh output on the blocks 0, 1, 2 and the two flow matches), rgb_atlas [6 N, 3] (F_Atlas's tanh
    output on the foreground, then the background queries of the blocks 0, 1, 2); `batch` from `atlas_batch`; cfg: the nine
    weights, uv_mapping_scale, derivative_amount, global_derivative_amount and with_alpha_loss by the field names of
    vsx_atlas_loss_cfg -> (losses [14] in the order ATLAS_LOSSES, g_uv_fg, g_uv_bg, g_alpha_raw, g_rgb_atlas).  No atomics:
    two calls give the same bits."""
    N = batch['rgb'].shape[0]
    B = batch['rows'].shape[0]
    for t, name, shape in ((uv_fg, 'uv_fg', (B * N, 2)), (uv_bg, 'uv_bg', (B * N, 2)), (rgb_atlas, 'rgb_atlas', (6 * N, 3))):
        _chk(t, name, torch.float32)
        if tuple(t.shape) != shape:
            raise _lib.VsxError(f'atlas_losses: {name} must be {list(shape)}, got {tuple(t.shape)}')
    _chk(alpha_raw, 'alpha_raw', torch.float32)
    if alpha_raw.numel() != 5 * N or alpha_raw.dim() > 2:
        raise _lib.VsxError(f'atlas_losses: alpha_raw must hold {5 * N} values, got {tuple(alpha_raw.shape)}')
    for k in ('rgb', 'rgb_dx', 'rgb_dy', 'alpha_gt', 'm_fwd', 'm_bwd'):
        _chk(batch[k], k, torch.float32)
    _chk(batch['counts'], 'counts', torch.int32)
    c = _lib.AtlasLossCfg()
    for k, _ in _lib.AtlasLossCfg._fields_:
        if k == 'larger_dim':
            c.larger_dim = int(batch['larger_dim'])
        elif k == 'with_global_rigidity':
            c.with_global_rigidity = int(B == 9)
        elif k in ('derivative_amount', 'global_derivative_amount', 'with_alpha_loss'):
            setattr(c, k, int(cfg[k]))
        else:
            setattr(c, k, float(cfg[k]))
    lib = _lib.load()
    dev = uv_fg.device
    losses = torch.empty(14, dtype=torch.float32, device=dev)
    grads = [torch.empty_like(t) for t in (uv_fg, uv_bg, alpha_raw, rgb_atlas)]
    scratch = torch.empty(lib.vsx_atlas_losses_workspace(N), dtype=torch.float32, device=dev)
    rc = lib.vsx_atlas_losses_f32(_p(uv_fg), _p(uv_bg), _p(alpha_raw), _p(rgb_atlas), N,
                                  *(_p(batch[k]) for k in ('rgb', 'rgb_dx', 'rgb_dy', 'alpha_gt', 'm_fwd', 'm_bwd', 'counts')),
                                  ctypes.byref(c), _p(losses), *(_p(g) for g in grads), _p(scratch), scratch.numel(), _stream())
    _check_supported(rc, 'vsx_atlas_losses_f32')
    return (losses, *grads)


def set_option(name, value):
    """Process-wide tuning / test switch of libvsx (the table in csrc/options.cpp).  The library holds the only copy: the
    host-side choices that depend on an option (`_conv_form`) ask the library, which reads it there."""
    check(_lib.load().vsx_set_option(name.encode(), int(value)), 'vsx_set_option')


def get_option(name):
    """The current value of a libvsx option (its environment variable's, or the default, until `set_option`)."""
    value = ctypes.c_int64()
    check(_lib.load().vsx_get_option(name.encode(), ctypes.byref(value)), 'vsx_get_option')
    return value.value


_prof_state = {'on': 0, 'max': 0, 'stride': 1, 'paused': False}


def prof_pause(paused):
    """Suspend / resume the hipEvent bracketing of GEMM launches (graph capture and graph-replayed calls)."""
    if paused == _prof_state['paused']:
        return
    _prof_state['paused'] = paused
    if _prof_state['on']:
        check(_lib.load().vsx_prof_pause(1 if paused else 0), 'vsx_prof_pause')


def prof_enable(on, max_samples=4096, stride=1):
    """Bracket every `stride`-th vsx_gemm_f16 launch with hipEvents (bench.py's roofline object)."""
    _prof_state.update(on=1 if on else 0, max=max_samples, stride=stride, paused=False)
    check(_lib.load().vsx_prof_enable((max(int(stride), 1) if on else 0), max_samples), 'vsx_prof_enable')


def prof_collect_roofline(peak_flops, peak_bytes_per_s):
    """-> dict(n, ms, flop, bytes, floor_ms, byte_bound_ms) over the sampled launches (include/vsx.h: vsx_prof_collect_roofline)"""
    n = ctypes.c_int64(0)
    v = [ctypes.c_double(0) for _ in range(5)]
    check(_lib.load().vsx_prof_collect_roofline(float(peak_flops), float(peak_bytes_per_s), ctypes.byref(n),
                                                *[ctypes.byref(x) for x in v]), 'vsx_prof_collect_roofline')
    return dict(n=n.value, ms=v[0].value, flop=v[1].value, bytes=v[2].value, floor_ms=v[3].value, byte_bound_ms=v[4].value)


def prof_collect():
    n = ctypes.c_int64(0)
    ms = ctypes.c_double(0)
    fl = ctypes.c_double(0)
    check(_lib.load().vsx_prof_collect(ctypes.byref(n), ctypes.byref(ms), ctypes.byref(fl)), 'vsx_prof_collect')
    return n.value, ms.value, fl.value


# --------------------------------------------------------------------------------------------
# kernel functions of the gradient path (adapter training step): csrc/train.hip, declared in
# include/vsx.h since ABI 5 (first run on hardware in round 3)
# --------------------------------------------------------------------------------------------
def _train_fn(name):
    return getattr(_lib.load(), name)


def geglu_fwd(y2):
    """y2 [.., 2N] = (h | g) pre-activations -> h * gelu_erf(g) [.., N] (the GEMM's GEGLU epilogue as its own pass: the
    gradient needs the pre-activations)."""
    _chk(y2, 'y2')
    n = y2.shape[-1] // 2
    out = torch.empty(*y2.shape[:-1], n, dtype=_F16, device=y2.device)
    check(_train_fn('vsx_geglu_fwd')(_p(y2), _p(out), y2.numel() // (2 * n), n, _stream()), 'vsx_geglu_fwd')
    return out


def geglu_bwd(dout, y2):
    """-> d y2 [.., 2N]: dh = dout * gelu(g), dg = dout * h * gelu'(g)."""
    _chk(dout, 'dout'); _chk(y2, 'y2')
    n = y2.shape[-1] // 2
    dy2 = torch.empty_like(y2)
    check(_train_fn('vsx_geglu_bwd')(_p(dout), _p(y2), _p(dy2), y2.numel() // (2 * n), n, _stream()), 'vsx_geglu_bwd')
    return dy2


def silu_bwd(dy, x):
    _chk(dy, 'dy'); _chk(x, 'x')
    dx = torch.empty_like(x)
    check(_train_fn('vsx_silu_bwd')(_p(dy), _p(x), _p(dx), x.numel(), _stream()), 'vsx_silu_bwd')
    return dx


def group_norm_bwd(dy, x, gamma, beta, groups, eps, nimg, silu=False, x2=None):
    """Data gradient of `group_norm` (same arguments; dy [.., C1+C2]) -> (dx [.., C1], dx2 [.., C2] or None)."""
    _chk(dy, 'dy'); _chk(x, 'x'); _chk(x2, 'x2'); _chk(gamma, 'gamma'); _chk(beta, 'beta')
    C1 = x.shape[-1]
    C2 = x2.shape[-1] if x2 is not None else 0
    rows = x.numel() // C1 // nimg
    dx = torch.empty_like(x)
    dx2 = torch.empty_like(x2) if x2 is not None else None
    ws = torch.empty(int(_train_fn('vsx_groupnorm_bwd_workspace')(nimg, rows, groups)), dtype=torch.float32, device=x.device)
    check(_train_fn('vsx_groupnorm_bwd')(_p(dy), _p(x), _p(x2), nimg, rows, C1, C2, groups, _p(gamma), _p(beta),
                                         float(eps), 1 if silu else 0, _p(ws), _p(dx), _p(dx2), _stream()),
          'vsx_groupnorm_bwd')
    return dx, dx2


def layer_norm_bwd(dy, x, gamma, eps=1e-5):
    """Data gradient of `layer_norm` (the positional encoding is added after the normalisation: it does not enter)."""
    _chk(dy, 'dy'); _chk(x, 'x'); _chk(gamma, 'gamma')
    C = x.shape[-1]
    dx = torch.empty_like(x)
    check(_train_fn('vsx_layernorm_bwd')(_p(dy), _p(x), _p(gamma), float(eps), _p(dx), x.numel() // C, C, _stream()),
          'vsx_layernorm_bwd')
    return dx


def softmax_bwd(probs, dprobs, scale):
    """dS = scale * P o (dP - rowsum(dP o P)), written over dP.  Both are views of row-padded buffers as
    `attention_scores` returns them ([nb, heads, nq, nk], row stride ld)."""
    nb, heads, nq, nk = probs.shape
    ld = probs.stride(2)
    if dprobs.shape != probs.shape or dprobs.stride() != probs.stride() or probs.stride(3) != 1:
        raise _lib.VsxError('softmax_bwd: probs and dprobs must share shape and (padded-row) strides')
    # the kernel walks nb*heads*nq rows of stride ld (the stride of an axis of size 1 is never used)
    if ld < nk or (heads > 1 and probs.stride(1) != nq * ld) or (nb > 1 and probs.stride(0) != heads * nq * ld):
        raise _lib.VsxError(f'softmax_bwd: rows must be evenly spaced (strides {probs.stride()} of shape {tuple(probs.shape)}): '
                            f'pass the whole buf[..., :nk] view, not a slice of its rows')
    _chk_view(probs, 'probs'); _chk_view(dprobs, 'dprobs')
    check(_train_fn('vsx_softmax_bwd')(_p(probs), _p(dprobs), nb * heads * nq, nk, ld, float(scale), _stream()),
          'vsx_softmax_bwd')
    return dprobs


def attention_bwd_supported(dh):
    """Head dims the flash-attention backward kernels exist for (csrc/attention_bwd.hip)."""
    return bool(_train_fn('vsx_attention_bwd_supported')(int(dh)))


def attention_lse(q, k, vt, heads, scale, kv_div=1, nk=None):
    """`attention` that also returns lse [nb, heads, round_up(nq, 64)] fp32 (log2 of the softmax denominators in the
    scaled-score domain, zero beyond nq): what `attention_bwd` recomputes the probabilities from."""
    _chk(vt, 'vt')
    ldq, q_bs = _rows_view(q, 'q')
    ldk, k_bs = _rows_view(k, 'k')
    nb, nq, C = q.shape
    nk = k.shape[1] if nk is None else nk
    dh = C // heads
    out = torch.empty(nb, nq, C, dtype=_F16, device=q.device)
    lds = round_up(nq, 64)
    lse = torch.zeros(nb, heads, lds, dtype=torch.float32, device=q.device)
    if FlopCounter.enabled:
        FlopCounter.attention += 4.0 * nb * heads * nq * nk * dh
    check(_train_fn('vsx_attention_lse_f16')(_p(q), _p(k), _p(vt), _p(out), _p(lse), lds, nb, heads, nq, nk, dh, ldq, ldk,
                                             vt.shape[2], C, q_bs, k_bs, C * vt.shape[2], nq * C, kv_div, float(scale),
                                             _stream()), 'vsx_attention_lse_f16')
    return out, lse


def attention_bwd(q, k, v, out, dout, lse, heads, scale, kv_div=1, need_kv=True):
    """Data gradients of the fused attention without the [heads, nq, nk] probabilities (csrc/attention_bwd.hip).
    q, out, dout [nb, nq, C]; k, v [nb / kv_div, nk, C], all contiguous; lse from `attention_lse`.
    -> (dq, dk, dv) (dk = dv = None unless need_kv; kv_div > 1: dq only)."""
    for t, n in ((q, 'q'), (k, 'k'), (v, 'v'), (out, 'out'), (dout, 'dout')):
        _chk(t, n)
    _chk(lse, 'lse', torch.float32)
    nb, nq, C = q.shape
    nk = k.shape[1]
    dh = C // heads
    lds = lse.shape[-1]

    def transposed(t):          # [n_img, n, C] -> [n_img, C, round_up(n, 8)], zero padded
        n = t.shape[1]
        ld = round_up(n, 8)
        tt = torch.zeros(t.shape[0], C, ld, dtype=_F16, device=t.device) if ld != n else \
            torch.empty(t.shape[0], C, ld, dtype=_F16, device=t.device)
        tt[:, :, :n] = t.transpose(1, 2)
        return tt
    kt = transposed(k)
    qt = dot = dk = dv = None
    if need_kv:
        if kv_div != 1:
            raise _lib.VsxError('attention_bwd: key / value gradients of a shared (text) context')
        qt, dot = transposed(q), transposed(dout)
        dk, dv = torch.empty_like(k), torch.empty_like(v)
    dq = torch.empty_like(q)
    delta = torch.empty(nb, heads, lds, dtype=torch.float32, device=q.device)
    check(_train_fn('vsx_attention_bwd_f16')(_p(q), _p(k), _p(v), _p(out), _p(dout), _p(qt), _p(kt), _p(dot), _p(lse),
                                             _p(delta), _p(dq), _p(dk), _p(dv), nb, heads, nq, nk, dh,
                                             qt.shape[2] if qt is not None else 0, kt.shape[2], lds, kv_div, float(scale),
                                             _stream()), 'vsx_attention_bwd_f16')
    return dq, dk, dv


def sum_pool2x2(x):
    """[n, 2h, 2w, c] -> [n, h, w, c]: the data gradient of the nearest-2x upsampling folded into a conv's loader."""
    _chk(x, 'x')
    n, h2, w2, c = x.shape
    if h2 % 2 or w2 % 2:             # the kernel strides the input by 2h and 2w
        raise _lib.VsxError(f'sum_pool2x2: height and width must be even, got {h2} x {w2}')
    y = torch.empty(n, h2 // 2, w2 // 2, c, dtype=_F16, device=x.device)
    check(_train_fn('vsx_sum_pool2x2')(_p(x), _p(y), n, h2 // 2, w2 // 2, c, _stream()), 'vsx_sum_pool2x2')
    return y


def adapter_gather(tracks, selected, dmap, rate, out_scale=1.0):
    """Gradient of `adapter_scatter` with respect to feat: dfeat[p, :] = out_scale * sum over frames and the 4 bilinear
    corners of weight * dmap[f, y, x, :] (same fp16 sub-pixel positions and weights as the forward)."""
    _chk(tracks, 'tracks', torch.float32); _chk(selected, 'selected', torch.int32); _chk(dmap, 'dmap')
    F, P = tracks.shape[:2]
    _, h, w, C = dmap.shape
    dfeat = torch.zeros(P, C, dtype=_F16, device=dmap.device)
    if P == 0:                       # an empty tensor has no address to hand to the entry point
        return dfeat
    check(_train_fn('vsx_adapter_gather')(_p(tracks), _p(selected), _p(dmap), _p(dfeat), F, P, C, h, w, float(rate),
                                          float(out_scale), _stream()), 'vsx_adapter_gather')
    return dfeat


# --------------------------------------------------------------------------------------------
# kernel table and gradient dispatch
# --------------------------------------------------------------------------------------------
# Every op above is a "kernel function" (it launches HIP kernels and nothing else).  The names the rest of the package
# calls are thin wrappers that (1) look the kernel function up in `_raw` at call time — one table a test harness can
# swap as a whole — and (2) when autograd is recording and an ACTIVATION argument requires grad (only the adapter
# training step, trainer_videoswap.py:33-97: the UNet's weights are frozen), route the call through the matching
# torch.autograd.Function of videoswap_amd/autograd.py, whose backward is again built from kernel functions.
_raw = {}

# op name -> positions / keywords of the arguments whose requires_grad switches the gradient path on: the activation
# arguments, and for `linear` also weight and bias (the adapter's MLPs are the trainable parameters of the training step:
# their first Linear gets an input WITHOUT grad — the point embedding — and must still record, adapter_model.py:70-107)
_ACTIVATIONS = {
    'linear': ((0, 1, 2), ('weight', 'bias', 'residual')), 'linear_vt': ((0,), ()), 'conv2d': ((0,), ('x2', 'residual')),
    'attention': ((0, 1, 2), ()), 'temporal_attention': ((0, 1, 2), ()), 'attention_scores': ((0, 1), ()),
    'attention_pv': ((0, 1), ()), 'head_scores': ((0, 1), ()), 'group_norm': ((0,), ('x2',)), 'layer_norm': ((0,), ()),
    'silu': ((0,), ()), 'quick_gelu': ((0,), ()), 'axpy': ((0, 1), ()), 'pack_latents': ((0,), ()),
    'unpack_latents': ((0,), ()), 'cfg_ddim_step': ((0, 1, 2), ()), 'masked_blend': ((0, 1), ()),
    'adapter_scatter': ((2,), ()),
}
_PLAIN = ('gemm', 'set_option', 'get_option', 'prof_pause', 'prof_enable', 'prof_collect', 'prof_collect_roofline', 'softmax_rows', 'geglu_fwd', 'geglu_bwd', 'silu_bwd',
          'group_norm_bwd', 'layer_norm_bwd', 'softmax_bwd', 'sum_pool2x2', 'adapter_gather', 'attention_lse',
          'attention_bwd', 'attention_bwd_supported', 'dift_sample_points', 'dift_cosine_map', 'coord_mlp', 'hash_grid',
          'hash_mlp', 'atlas_edit', 'coord_mlp_train_workspace', 'coord_mlp_train_forward', 'coord_mlp_backward',
          'hash_grid_backward', 'hash_mlp_train_workspace', 'hash_mlp_train_forward', 'hash_mlp_backward', 'atlas_batch',
          'atlas_losses')


def _publish(name):
    _raw[name] = globals()[name]
    pos, kws = _ACTIVATIONS.get(name, ((), ()))

    def op(*args, **kwargs):
        if pos and torch.is_grad_enabled():
            for i in pos:
                if i < len(args) and torch.is_tensor(args[i]) and args[i].requires_grad:
                    break
            else:
                for k in kws:
                    t = kwargs.get(k)
                    if t is not None and t.requires_grad:
                        break
                else:
                    return _raw[name](*args, **kwargs)
            from . import autograd
            # the gradient path works on plain tensors: a LayerNorm deferred into this consumer (its own input had no
            # gradient, e.g. unfrozen weights under grad mode) is applied by its standalone kernel first
            if args and isinstance(args[0], DeferredLN):
                args = (args[0].materialize(),) + tuple(args[1:])
            return autograd.dispatch(name, *args, **kwargs)
        return _raw[name](*args, **kwargs)

    op.__name__ = name
    op.__doc__ = _raw[name].__doc__
    globals()[name] = op


for _name in tuple(_ACTIVATIONS) + _PLAIN:
    _publish(_name)
del _name
