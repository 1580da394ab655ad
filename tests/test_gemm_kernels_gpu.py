"""GPU parity tests of vsx_gemm_f16 (videoswap_amd/csrc/gemm.hip, gemm_pp.hip): the six workgroup-per-tile kernels, split-K and its
combine kernel, the persistent 256- and 128-row kernels, the weight-stationary K = 320 kernel, both convolution loaders and the
sub-pixel form, under every epilogue — each case aimed at one kernel's edge through the plan query (vsx_gemm_plan), which the runner
asserts before it launches.

Cases, references and the rule live in tests/gemm_case.py (shared with their CPU proof, tests/test_gemm_case.py).  Inputs E: small
integers, on which the stored bits must equal the fp64 result rounded to fp16 once; Inputs R (GEGLU, the fold with a real rstd, a
residual 64 x the product): train_kernel_case.measure against fp64 and the fp32 ideal.  In every case C lies inside a sentinel-filled
buffer that must come back untouched outside the result, and A and B carry eight pad columns of 60000 behind K.  Cases build
ops.GemmDesc themselves and go through ops.gemm; a few go through ops.linear / linear_vt / conv2d / DeferredLN for the wrappers' own
arithmetic.  Figures: profiles/gemm_parity.json (VSX_WRITE_PROFILES=1).
"""
import json
import os
import time

import pytest
import torch

import gemm_case as gc
from util import ROOT

pytestmark = pytest.mark.gpu
DEV = 'cuda'
T0 = [None]


class GpuImpl(gc.LibQueries):
    def __init__(self):
        super().__init__()
        from videoswap_amd import ops
        self.ops = ops
        self.DeferredLN, self.linear, self.linear_vt = ops.DeferredLN, ops.linear, ops.linear_vt

    def gemm(self, d):
        self.ops.gemm(d)

    def sync(self):
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:                # a fault on the device: nothing more is started on it
            pytest.exit(f'the device reported {e}', returncode=3)

    def conv2d_form(self, subpixel, x, w, b, upsample):
        """ops.conv2d in the form asked for; the FLOP counter says which one ran (the sub-pixel form skips five taps of nine)"""
        o = self.ops
        saved = o.CONV_SUBPIXEL
        o.CONV_SUBPIXEL = subpixel
        o.FlopCounter.reset(True)
        try:
            y = o.conv2d(x, w, b, upsample=upsample)
            assert (o.FlopCounter.gemm_saved > 0) == subpixel, 'ops.conv2d took the other form'
            return y
        finally:
            o.CONV_SUBPIXEL = saved
            o.FlopCounter.reset(False)


_impl = []


def impl():
    if not _impl:
        _impl.append(GpuImpl())
        T0[0] = time.time()
    return _impl[0]


@pytest.mark.parametrize('c', gc.TILE_CASES, ids=gc.case_id)
def test_tile_kernels(c):
    gc.run_case(impl(), DEV, c)


def test_xcd_block_grid_equals_the_linear_walk():
    """the same launch under xcd_walk 0 and 1: the walk decides which workgroup computes a tile, never a bit of the result"""
    for name in ('tile6-xcd{}-256x256x72', 'tile2-xcd{}-1024x640x136'):
        outs = []
        for walk in (0, 1):
            c = dict(gc.BY_NAME[name.format(walk)], name=name.format('*'))          # (one name: the same inputs)
            with gc.options(impl(), c['opts']):
                pb = gc.build(c, DEV, impl())
                gc.assert_plan(impl(), pb)
                impl().gemm(pb.d)
                impl().sync()
                outs.append(pb.cbuf.cpu())
        assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), name


@pytest.mark.parametrize('c', gc.SPLIT_CASES, ids=gc.case_id)
def test_split_k(c):
    gc.run_case(impl(), DEV, c)


@pytest.mark.parametrize('c', gc.PP_CASES, ids=gc.case_id)
def test_persistent_kernels(c):
    gc.run_case(impl(), DEV, c)


@pytest.mark.parametrize('c', gc.WS_CASES, ids=gc.case_id)
def test_weight_stationary_kernel(c):
    gc.run_case(impl(), DEV, c)


@pytest.mark.parametrize('c', gc.CONV_CASES, ids=gc.case_id)
def test_convolution_loaders(c):
    gc.run_case(impl(), DEV, c)


@pytest.mark.parametrize('c', gc.SUBPIXEL_CASES, ids=gc.case_id)
def test_sub_pixel_form(c):
    gc.run_case(impl(), DEV, c)


@pytest.mark.parametrize('c', gc.R_CASES, ids=gc.case_id)
def test_rounded_inputs(c):
    gc.run_case(impl(), DEV, c)


@pytest.mark.parametrize('c', gc.REFUSALS, ids=gc.case_id)
def test_refusals_just_below_the_smallest_eligible_shape(c):
    assert gc.run_case(impl(), DEV, c) is None


@pytest.mark.parametrize('name', gc.WRAPPER_RUNS)
def test_wrappers(name):
    gc.run_wrapper(impl(), DEV, name)


def test_options_are_back_at_their_defaults():
    for name, default in (('gemm_pp', 1), ('gemm_ws', 1), ('ws_waves', 10), ('xcd_walk', 1), ('conv_winograd', 1), ('tile_tune', 0), ('pp_sched', 0)):
        env = os.environ.get({'gemm_pp': 'VSX_GEMM_PP', 'gemm_ws': 'VSX_GEMM_WS', 'ws_waves': 'VSX_WS_WAVES', 'xcd_walk': 'VSX_XCD_WALK',
                              'conv_winograd': 'VSX_CONV_WINOGRAD', 'tile_tune': 'VSX_TUNE_TILE', 'pp_sched': 'VSX_PP_SCHED'}[name])
        assert impl().get_option(name) == (default if env is None else int(env)), name


def test_parity_figures_recorded():
    """runs after the parity cases (file order): each left its figure; VSX_WRITE_PROFILES=1 writes the profile"""
    figs = gc.FIGURES
    assert len(figs) == gc.expected_figures() + sum(n.startswith('deferred-ln') for n in gc.WRAPPER_RUNS)
    exact = [f for f in figs if f['cls'] == 'E']
    rounded = [f for f in figs if f['cls'] == 'R']
    assert all(f['mismatches'] == 0 for f in exact)
    worst = {m: max((f[m + '_kernel'] / f[m + '_bound'], f['case']) for f in rounded if f[m + '_bound'] > 0) for m in ('l2', 'row', 'maxabs', 'elem')}
    summary = dict(exact_cases=len(exact), exact_elements=sum(f['elements'] for f in exact), exact_ties=sum(f['ties'] for f in exact),
                   rounded_cases=len(rounded), worst_ratio_to_bound={m: dict(ratio=r, case=c) for m, (r, c) in worst.items()},
                   wall_seconds=time.time() - T0[0])
    print(json.dumps(summary, indent=1))
    if os.environ.get('VSX_WRITE_PROFILES') == '1':
        out = os.environ.get('VSX_PROFILE_DIR', os.path.join(ROOT, 'profiles'))
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, 'gemm_parity.json'), 'w') as f:
            json.dump({'device': torch.cuda.get_device_name(0), 'rule': gc.RULE, 'summary': summary, 'rounded': rounded,
                       'exact': [dict(case=f['case'], elements=f['elements'], ties=f['ties'], mismatches=f['mismatches'],
                                      **({'stat_rows_wrong': f['stat_rows_wrong']} if 'stat_rows_wrong' in f else {})) for f in exact]}, f, indent=1)
