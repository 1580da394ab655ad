"""Winograd F(2x2, 3x3) form of the stride-1 3x3 convolutions on the GPU (csrc/winograd.hip through videoswap_amd.ops.conv2d)
against F.conv2d in fp32 and against the direct kernels on the same inputs.

Inputs are those of tests/winograd_case.py: SiLU of unit-variance noise (what a resnet convolution reads behind GroupNorm + SiLU),
weights ~ N(0, 1 / K), and the epilogue terms the resnets' convolutions carry (conv1: bias + time-embedding row vector; conv2:
bias + residual).  Bounds: the project's 2e-3 for a convolution, and 3 x the direct kernel's error on the same inputs.

Measured on an MI355X (direct 2.07 - 2.08e-4 everywhere): bias + row vector 5.5e-4 (2.65 - 2.67 x), with a residual 3.5e-4 (1.66 x)."""
import functools

import pytest
import torch

import winograd_case as wc
from test_winograd import _desc

pytestmark = pytest.mark.gpu

# nimg, H, W, C1, C2, Cout, rowvec, residual, forced
SHAPES = [
    (2, 8, 8, 640, 0, 1280, True, False, False),
    (1, 16, 16, 1280, 1280, 1280, True, True, False),
    (3, 4, 6, 64, 0, 64, False, True, True),            # below the automatic thresholds: forced through the option
    (3, 16, 16, 640, 0, 1280, True, False, False),      # M / 4 = 192: not a multiple of the GEMM's 128-row tiles
]


@functools.lru_cache(maxsize=None)
def _case(shape):
    nimg, H, W, C1, C2, Cout, rowvec, residual, _ = shape
    case = wc.make_case(nimg, H, W, C1, C2, Cout, rowvec=rowvec, residual=residual, seed=7)
    ref = wc.reference(case, torch.float32)             # computed once per shape, shared, never written
    dev = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in case.items()}
    return dev, ref


def _conv(ops, c):
    return ops.conv2d(c['x'], c['weight'], c['bias'], x2=c['x2'], rowvec=c['rowvec'], rows_per_vec=c['rows_per_vec'],
                      residual=c['residual'])


@pytest.fixture
def ops():
    from videoswap_amd import ops as _ops
    saved = _ops.get_option('conv_winograd')
    yield _ops
    _ops.set_option('conv_winograd', saved)


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(str(int(v)) for v in s))
def test_winograd_convolution_against_fp32_and_the_direct_kernels(ops, shape):
    c, ref = _case(shape)
    forced = shape[-1]
    ops.set_option('conv_winograd', 2 if forced else 1)
    assert ops._conv_form(_desc(*shape[:6])) == 'winograd'
    assert forced or shape[3] + shape[4] >= 640          # the unforced shapes take the form under the automatic rule
    launches = []
    real = ops._conv_winograd
    ops._conv_winograd = lambda *a: (launches.append(1), real(*a))[1]
    try:
        out = _conv(ops, c)
        again = _conv(ops, c)
    finally:
        ops._conv_winograd = real
    assert len(launches) == 2                            # the form under test did run, both times
    ops.set_option('conv_winograd', 0)
    direct = _conv(ops, c)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    err, derr = wc.rel_l2(out.cpu(), ref), wc.rel_l2(direct.cpu(), ref)
    print(f'winograd rel-L2 {err:.3e}  direct {derr:.3e}  ratio {err / derr:.2f}')
    assert err < wc.REL_L2_BOUND
    assert err <= wc.RATIO_BOUND * derr
    assert torch.equal(out, again)                       # two calls agree bit for bit


def test_an_unsupported_description_is_refused(ops):
    from videoswap_amd import _lib
    import ctypes
    c, _ = _case(SHAPES[2])
    x = c['x'][:, :, :5].contiguous()                    # odd W
    d = _lib.GemmDesc()
    d.M, d.N, d.K = 3 * 4 * 5, 64, 9 * 64
    d.batch0 = d.batch1 = 1
    out = torch.empty(3, 4, 5, 64, dtype=torch.float16, device='cuda')
    d.A, d.B, d.C = x.data_ptr(), c['weight'].data_ptr(), out.data_ptr()
    d.a_mode, d.H, d.W, d.C1, d.ks, d.stride = 1, 4, 5, 64, 3, 1
    d.ldb, d.ldc, d.alpha = d.K, 64, 1.0
    lib = _lib.load()
    assert lib.vsx_conv3x3_winograd_workspace(ctypes.byref(d)) == 0
    u = ops.winograd_weights(c['weight'])
    ws = torch.empty(1 << 16, dtype=torch.float16, device='cuda')
    rc = lib.vsx_conv3x3_winograd_f16(ctypes.byref(d), u.data_ptr(), ws.data_ptr(), ws.numel() * 2, None)
    assert rc == _lib.VSX_E_UNSUPPORTED and b'even' in lib.vsx_last_error()
    # and conv2d itself takes the direct kernels for it, whatever the option says
    ops.set_option('conv_winograd', 2)
    assert ops._conv_form(_desc(3, 4, 5, 64, 0, 64)) == 'direct'
    y = ops.conv2d(x, c['weight'], c['bias'])
    ref = wc.reference(dict(x=x.cpu(), x2=None, weight=c['weight'].cpu(), bias=c['bias'].cpu(), rowvec=None, residual=None),
                       torch.float32)
    assert wc.rel_l2(y.cpu(), ref) < wc.REL_L2_BOUND
