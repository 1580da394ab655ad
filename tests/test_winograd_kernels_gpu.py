"""GPU parity tests of vsx_conv3x3_winograd_f16 (videoswap_amd/csrc/winograd.hip: the input transform, the batched vsx_gemm_f16
launch, the output transform with its epilogue) stage by stage, each case aimed at one indexing edge.

Cases, references and the rule live in tests/winograd_case.py (shared with their CPU proof, tests/test_winograd_case.py).  The
workspace is the caller's and is never cleared, so V and Mt are read back after every call and each stage is judged on the
kernel's own input to it: V and Y bit-equal to fp32 restatements in the kernels' written order, Mt under gemm_case's rule, and on
Inputs E (small integers) every stage bit-equal to fp64.  C and a workspace of exactly the size the library asks for lie inside
sentinel-filled buffers that must come back untouched outside the result; ldc > N, ldr != ldc.  Cases build the GemmDesc
themselves and call the entry point; a few go through ops.conv2d.  Figures: profiles/winograd_parity.json (VSX_WRITE_PROFILES=1).
"""
import ctypes
import json
import os
import time

import pytest
import torch

import winograd_case as wc
from util import ROOT

pytestmark = pytest.mark.gpu
DEV = 'cuda'
T0 = [None]


class GpuImpl(wc.WinoQueries):
    def __init__(self):
        super().__init__()
        from videoswap_amd import ops
        self.ops = ops
        self.winograd_weights = ops.winograd_weights

    def winograd(self, d, u_ptr, ws_ptr, ws_bytes):
        return int(self.lib().vsx_conv3x3_winograd_f16(ctypes.byref(d), ctypes.c_void_p(u_ptr), ctypes.c_void_p(ws_ptr), ws_bytes,
                                                       self.ops._stream()))

    def gemm(self, d):
        self.ops.gemm(d)

    def sync(self):
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:                # a fault on the device: nothing more is started on it
            pytest.exit(f'the device reported {e}', returncode=3)

    def conv2d(self, x, weight, bias=None, **kw):
        """ops.conv2d, and how many times it launched the Winograd form"""
        o = self.ops
        launches = []
        real = o._conv_winograd
        o._conv_winograd = lambda *a: (launches.append(1), real(*a))[1]
        try:
            return o.conv2d(x, weight, bias, **kw), len(launches)
        finally:
            o._conv_winograd = real


_impl = []


def impl():
    if not _impl:
        _impl.append(GpuImpl())
        T0[0] = time.time()
    return _impl[0]


@pytest.mark.parametrize('c', wc.GEOMETRY_CASES, ids=wc.case_id)
def test_image_geometry(c):
    wc.run_case(impl(), DEV, c)


@pytest.mark.parametrize('c', wc.CHANNEL_CASES, ids=wc.case_id)
def test_channels(c):
    wc.run_case(impl(), DEV, c)


@pytest.mark.parametrize('c', wc.EPILOGUE_CASES, ids=wc.case_id)
def test_epilogue(c):
    wc.run_case(impl(), DEV, c)


@pytest.mark.parametrize('c', wc.ROUNDED_CASES, ids=wc.case_id)
def test_rounded_inputs(c):
    wc.run_case(impl(), DEV, c)


@pytest.mark.parametrize('c', wc.WRAPPER_CASES, ids=wc.case_id)
def test_through_conv2d(c):
    wc.run_wrapper(impl(), DEV, c)


@pytest.mark.parametrize('r', wc.REFUSALS, ids=lambda r: r[0])
def test_refusals_one_step_outside_the_supported_set(r):
    wc.run_refusal(impl(), DEV, r)


def test_large_index_case_on_a_sample_of_tiles():
    """M (C1 + C2) one step below 2^31: the xi planes of V and the batch offsets of the GEMM pass 2^31 elements (23 GB on the device)"""
    wc.run_large(impl(), DEV, wc.LARGE)
    torch.cuda.empty_cache()


def test_options_are_back_at_their_defaults():
    for name, default in (('gemm_pp', 1), ('gemm_ws', 1), ('ws_waves', 10), ('xcd_walk', 1), ('conv_winograd', 1), ('tile_tune', 0), ('pp_sched', 0)):
        env = os.environ.get({'gemm_pp': 'VSX_GEMM_PP', 'gemm_ws': 'VSX_GEMM_WS', 'ws_waves': 'VSX_WS_WAVES', 'xcd_walk': 'VSX_XCD_WALK',
                              'conv_winograd': 'VSX_CONV_WINOGRAD', 'tile_tune': 'VSX_TUNE_TILE', 'pp_sched': 'VSX_PP_SCHED'}[name])
        assert impl().get_option(name) == (default if env is None else int(env)), name


def test_parity_figures_recorded():
    """runs after the parity cases (file order): each left its figure; VSX_WRITE_PROFILES=1 writes the profile"""
    figs = wc.FIGURES
    assert len(figs) == wc.expected_figures() + 1           # + the large-index case
    exact = [f for f in figs if f['cls'] == 'E']
    rounded = [f for f in figs if f['cls'] == 'R']
    stages = ('u_mismatches', 'v_mismatches', 'v_mismatches_fp64', 'mt_mismatches', 'y_mismatches', 'y_mismatches_fp64', 'repeat_mismatches')
    assert all(f.get(k, 0) == 0 for f in figs for k in stages)
    worst = {m: max((f[f'mt_{m}_kernel'] / f[f'mt_{m}_bound'], f['case']) for f in rounded if f[f'mt_{m}_bound'] > 0) for m in ('l2', 'row', 'maxabs', 'elem')}
    worst['u'] = max((f['u_ratio'], f['case']) for f in rounded)
    worst['rel_l2'] = max((f['rel_l2'] / f['rel_l2_bound'], f['case']) for f in rounded)
    worst['ratio_to_direct'] = max((f['ratio_to_direct'] / f['ratio_bound'], f['case']) for f in rounded)
    summary = dict(exact_cases=len(exact), exact_elements=sum(f['elements'] for f in exact), exact_ties=sum(f['ties'] for f in exact),
                   rounded_cases=len(rounded), worst_ratio_to_bound={m: dict(ratio=r, case=c) for m, (r, c) in worst.items()},
                   slowest_case=max((f['wall_seconds'], f['case']) for f in figs), wall_seconds=time.time() - T0[0])
    print(json.dumps(summary, indent=1))
    if os.environ.get('VSX_WRITE_PROFILES') == '1':
        out = os.environ.get('VSX_PROFILE_DIR', os.path.join(ROOT, 'profiles'))
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, 'winograd_parity.json'), 'w') as f:
            json.dump({'device': torch.cuda.get_device_name(0), 'rule': wc.RULE, 'summary': summary, 'rounded': rounded, 'exact': exact}, f, indent=1)
