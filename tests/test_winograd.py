"""Host side of the Winograd F(2x2, 3x3) form of the stride-1 3x3 convolutions (include/vsx.h: vsx_conv3x3_winograd_f16;
csrc/winograd.hip).  No GPU: a torch restatement of the three stages with the kernels' rounding points against F.conv2d in
fp64, where `conv2d` takes the form (the library's rule, on both sides of every threshold and under every option set), and the
weight cache."""
import ctypes
import gc

import pytest
import torch

import winograd_case as wc
from videoswap_amd import _lib, ops


@pytest.mark.parametrize('nimg,H,W,C,Cout', [(3, 4, 6, 64, 64), (2, 8, 8, 640, 1280)])
def test_three_stages_with_the_kernels_rounding_points_against_fp64(nimg, H, W, C, Cout):
    case = wc.make_case(nimg, H, W, C, 0, Cout, rowvec=True, residual=False)
    ref = wc.reference(case)
    got = wc.winograd_restated(case)
    err, direct = wc.rel_l2(got, ref), wc.rel_l2(wc.direct_fp16(case), ref)
    print(f'winograd {err:.3e}  direct (one fp16 rounding) {direct:.3e}  ratio {err / direct:.2f}')
    assert err < wc.REL_L2_BOUND and err <= wc.RATIO_BOUND * direct
    # the transforms alone are exact identities in higher precision: the difference above is rounding, not algebra
    x = case['x']
    v = torch.einsum('ar,nijcrs,bs->abnijc', wc.BT.double(),
                     torch.nn.functional.pad(x.double(), (0, 0, 1, 1, 1, 1)).unfold(1, 4, 2).unfold(2, 4, 2), wc.BT.double())
    u = torch.einsum('ar,orsc,bs->aboc', wc.G.double(), case['weight'].double(), wc.G.double())
    m = torch.einsum('abnijc,aboc->abnijo', v, u)
    y = torch.einsum('pa,abnijo,qb->nipjqo', wc.AT.double(), m, wc.AT.double()).reshape(nimg, H, W, Cout)
    y = y + case['bias'].double() + case['rowvec'].double()[:, None, None, :]
    assert wc.rel_l2(y, ref) < 1e-12


def test_winograd_weights_are_the_transform_and_are_cached_per_weight_version():
    w = (torch.randn(8, 3, 3, 16) * 0.2).half()
    a = ops.winograd_weights(w)
    assert a.shape == (16, 8, 16) and a.dtype == torch.float16 and a.is_contiguous()
    assert torch.equal(a, wc.weight_transform(w))
    assert torch.equal(a[0], w[:, 0, 0]) and torch.equal(a[15], w[:, 2, 2])      # G's first and last rows pick the corners
    assert ops.winograd_weights(w) is a                 # same tensor object, same version: the cached copy
    assert any(t is a for t in ops.fold_cache_tensors())                         # what a captured graph holds on to
    w.mul_(2)                                           # anything that rewrites the weight in place bumps the version
    b = ops.winograd_weights(w)
    assert b is not a and torch.allclose(b.float(), 2 * a.float(), atol=2e-3, rtol=2e-3)
    key = id(w)
    del w, a, b
    gc.collect()
    assert key not in ops._winograd_cache               # the entry lives exactly as long as its weight


def _desc(nimg, H, W, C1, C2, Cout, ks=3, stride=1, upsample=0, padding=None):
    d = _lib.GemmDesc()
    d.M, d.N, d.K = nimg * H * W, Cout, ks * ks * (C1 + C2)
    d.batch0 = d.batch1 = 1
    d.A = 4096
    d.A2 = 8192 if C2 else None
    d.B, d.C = 12288, 16384
    d.a_mode, d.H, d.W, d.C1, d.C2 = 1, H, W, C1, C2
    d.ks, d.stride, d.upsample = ks, stride, upsample
    d.ldb, d.ldc, d.alpha = d.K, Cout, 1.0
    if padding is not None:
        d.pad_lo, d.pad_hi = padding
    return d


CASES = [
    # nimg, H, W, C1, C2, Cout, ks, stride, upsample, padding
    (16, 16, 16, 1280, 0, 1280, 3, 1, 0, None),         # the enabled set: 16 x 16 and 8 x 8 from 640 channels
    (32, 16, 16, 1280, 1280, 1280, 3, 1, 0, None),
    (16, 8, 8, 640, 0, 1280, 3, 1, 0, None),
    (16, 16, 16, 632, 0, 1280, 3, 1, 0, None),          # one octet below the channel threshold
    (16, 16, 16, 320, 320, 1280, 3, 1, 0, None),        # the threshold counts both sources
    (16, 16, 16, 320, 256, 1280, 3, 1, 0, None),
    (16, 16, 18, 640, 0, 1280, 3, 1, 0, None),          # H * W = 288: above the size threshold of 640 .. 1279 channels
    (16, 2, 128, 640, 0, 640, 3, 1, 0, None),           # H * W = 256 exactly
    (16, 32, 32, 640, 0, 640, 3, 1, 0, None),           # the 32 x 32 level: from 1280 input channels only
    (16, 32, 32, 640, 640, 640, 3, 1, 0, None),
    (16, 32, 32, 640, 576, 640, 3, 1, 0, None),
    (16, 32, 34, 1280, 0, 640, 3, 1, 0, None),          # H * W = 1088: above that level's size threshold
    (16, 64, 64, 1280, 0, 320, 3, 1, 0, None),
    (16, 16, 15, 1280, 0, 1280, 3, 1, 0, None),         # odd W / odd H: not supported
    (16, 15, 16, 1280, 0, 1280, 3, 1, 0, None),
    (16, 16, 16, 1284, 0, 1280, 3, 1, 0, None),         # channels not a multiple of 8
    (16, 16, 16, 1280, 0, 1284, 3, 1, 0, None),
    (16, 16, 16, 1280, 72, 1280, 3, 1, 0, None),        # two sources need multiples of 64
    (16, 16, 16, 1280, 0, 1280, 1, 1, 0, None),         # 1 x 1, stride 2, upsampling, one-sided padding
    (16, 16, 16, 1280, 0, 1280, 3, 2, 0, None),
    (16, 16, 16, 1280, 0, 1280, 3, 1, 1, None),
    (16, 16, 16, 1280, 0, 1280, 3, 1, 0, (0, 1)),
    (16, 16, 16, 1280, 0, 1280, 3, 1, 0, (1, 1)),       # the symmetric padding written out
    (3, 4, 6, 64, 0, 64, 3, 1, 0, None),                # supported, small: only when forced
]


def _takes_winograd(case):
    return ops._conv_form(_desc(*case)) == 'winograd'


def test_the_form_runs_where_the_library_rule_says_on_both_sides_of_every_threshold():
    """What `conv2d` takes (`ops._conv_form`) under every option set, against the rule as csrc/options.cpp states it."""
    lib = _lib.load()
    names = ('conv_winograd', 'gemm_pp', 'tile_tune')
    saved = {name: ops.get_option(name) for name in names}
    supported = []                                       # the rows the form takes at all: a workspace size > 0, by the formula
    for i, case in enumerate(CASES):
        nimg, H, W, C1, C2, Cout = case[:6]
        need = int(lib.vsx_conv3x3_winograd_workspace(ctypes.byref(_desc(*case))))
        if need:
            assert need == 16 * (nimg * H * W // 4) * (C1 + C2 + Cout) * 2
            supported.append(i)
    assert supported == [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 22, 23]
    # under the defaults: the enabled set, the rows exactly on a threshold and the written-out padding, nothing else
    enabled = [0, 1, 2, 4, 7, 9, 22]
    expect = [({}, enabled), ({'conv_winograd': 0}, []), ({'conv_winograd': 2}, supported),
              ({'conv_winograd': 2, 'gemm_pp': 0}, supported),
              ({'gemm_pp': 0}, []), ({'gemm_pp': 2}, []), ({'tile_tune': 2}, [])]      # mode 1 stays out of a forced back end's way
    try:
        for opts, want in expect:
            for name in names:
                ops.set_option(name, {**{'conv_winograd': 1, 'gemm_pp': 1, 'tile_tune': 0}, **opts}[name])
            assert [i for i, c in enumerate(CASES) if _takes_winograd(c)] == want, opts
            assert [i for i, c in enumerate(CASES) if lib.vsx_conv3x3_winograd_auto(ctypes.byref(_desc(*c)))] == want, opts
    finally:
        for name in names:
            ops.set_option(name, saved[name])


def test_the_gradient_path_keeps_the_direct_kernels():
    case = CASES[0]
    assert _takes_winograd(case)
    with ops.winograd_suspended():
        assert not _takes_winograd(case)
        with ops.winograd_suspended():
            assert not _takes_winograd(case)
        assert not _takes_winograd(case)
    assert _takes_winograd(case)
    import inspect
    from videoswap_amd import autograd
    assert inspect.getsource(autograd._Conv2d).count('winograd_suspended') == 2          # the forward and the dgrad launches


def test_an_unsupported_description_is_refused_without_touching_memory():
    lib = _lib.load()
    for case in (CASES[13], CASES[19], CASES[20], CASES[21]):
        d = _desc(*case)
        rc = lib.vsx_conv3x3_winograd_f16(ctypes.byref(d), ctypes.c_void_p(4096), ctypes.c_void_p(4096), 1 << 40, None)
        assert rc == _lib.VSX_E_UNSUPPORTED, case
    d = _desc(*CASES[0])
    d.geglu = 1
    assert lib.vsx_conv3x3_winograd_f16(ctypes.byref(d), ctypes.c_void_p(4096), ctypes.c_void_p(4096), 1 << 40, None) == _lib.VSX_E_UNSUPPORTED
    d = _desc(*CASES[0])                                 # a workspace that is too small is refused before any launch
    assert lib.vsx_conv3x3_winograd_f16(ctypes.byref(d), ctypes.c_void_p(4096), ctypes.c_void_p(4096), 1024, None) == -4
