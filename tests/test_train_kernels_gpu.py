"""GPU parity tests of the training-step kernels (videoswap_amd/csrc/train.hip) and of quick_gelu, silu and the two row
softmaxes, each on its own against an fp64 reference, at the smallest shapes that reach every path of each kernel.

Cases, references and the comparison rule live in tests/train_kernel_case.py (shared with the CPU proof of the rule,
tests/test_train_kernel_case.py).  Every bound is taken from the fp32 ideal on the same inputs; nothing is tuned to what the
kernels give.  Every call goes through videoswap_amd.ops.  Figures: profiles/train_kernel_parity.json (VSX_WRITE_PROFILES=1).
"""
import json
import os

import pytest
import torch

import train_kernel_case as tk
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


@pytest.mark.parametrize('run', tk.gn_runs(), ids=tk.gn_id)
def test_group_norm_bwd(run):
    tk.run_group_norm_bwd(ops(), DEV, run)


def test_group_norm_bwd_refusals():
    def call(nimg, rows, C1, C2, groups):
        z = (lambda *s: torch.zeros(*s, dtype=H, device=DEV))
        return ops().group_norm_bwd(z(nimg, rows, C1 + C2), z(nimg, rows, C1), z(C1 + C2), z(C1 + C2), groups, 1e-5, nimg,
                                    x2=z(nimg, rows, C2) if C2 else None)
    for shape in ((1, 4, 4104, 0, 8),            # C beyond the two LDS arrays
                  (1, 4, 2056, 0, 257),          # more groups than the finalize grid is written for
                  (1, 4, 12, 0, 4), (1, 4, 16, 12, 4),   # a source that is no multiple of the 16-byte vector
                  (1, 4, 64, 0, 3)):             # groups do not divide C
        with pytest.raises(vsx_error()):
            call(*shape)
    dx, _ = call(1, 4, 64, 0, 4)                  # the same call with a legal shape goes through
    assert dx.shape == (1, 4, 64)


@pytest.mark.parametrize('case', tk.LN_CASES, ids=lambda c: f'{c[0]}x{c[1]}-mean{c[2]:g}')
def test_layer_norm_bwd(case):
    tk.run_layer_norm_bwd(ops(), DEV, case)


@pytest.mark.parametrize('case', tk.SMB_CASES, ids=lambda c: 'x'.join(str(v) for v in c[:4]) + f'-scale{c[4]:.3f}')
def test_softmax_bwd(case):
    tk.run_softmax_bwd(ops(), DEV, case)


def test_softmax_bwd_refuses_views_with_uneven_rows():
    """the kernel walks nb * heads * nq rows of ONE stride: a slice of the query axis must not reach it"""
    pbuf, dbuf = tk.smb_inputs((2, 8, 9, 77, 1.0), DEV)
    before = dbuf.clone()
    with pytest.raises(vsx_error()):
        ops().softmax_bwd(pbuf[:, :, :8, :77], dbuf[:, :, :8, :77], 1.0)
    with pytest.raises(vsx_error()):
        ops().softmax_bwd(pbuf[..., :77], dbuf[..., :76], 1.0)
    assert torch.equal(dbuf, before)


@pytest.mark.parametrize('case', tk.GEGLU_CASES, ids=lambda c: f'{c[0]}x{c[1]}')
def test_geglu(case):
    tk.run_geglu(ops(), DEV, case)


def test_geglu_fwd_equals_the_gemm_epilogue_bit_for_bit():
    """csrc/common.h: every GEGLU path evaluates the same form.  An identity weight makes the GEMM hand y2 itself to its epilogue."""
    y2, _ = tk.geglu_inputs((37, 24), DEV)
    eye = torch.eye(48, dtype=H, device=DEV)
    assert torch.equal(ops().linear(y2, eye, geglu=True), ops().geglu_fwd(y2))


@pytest.mark.parametrize('n', tk.ACT_SIZES)
def test_silu_quick_gelu_silu_bwd(n):
    tk.run_activations(ops(), DEV, n)


@pytest.mark.parametrize('case', tk.POOL_CASES, ids=lambda c: 'x'.join(str(v) for v in c))
def test_sum_pool2x2(case):
    tk.run_sum_pool(ops(), DEV, case)


def test_sum_pool2x2_refuses_odd_sizes():
    for shape in ((1, 3, 4, 8), (1, 4, 5, 8), (2, 7, 7, 16)):
        with pytest.raises(vsx_error()):
            ops().sum_pool2x2(torch.zeros(*shape, dtype=H, device=DEV))


@pytest.mark.parametrize('C', tk.GATHER_C)
def test_adapter_gather(C):
    tk.run_adapter_gather(ops(), DEV, C)


def test_adapter_gather_without_points():
    tk.run_adapter_gather_empty(ops(), DEV)


def test_adapter_gather_is_the_adjoint_of_adapter_scatter():
    tk.run_adapter_adjoint(ops(), DEV)


@pytest.mark.parametrize('causal', [False, True], ids=['plain', 'causal'])
@pytest.mark.parametrize('ncols', tk.SMR_COLS)
def test_softmax_rows(ncols, causal):
    tk.run_softmax_rows(ops(), DEV, ncols, causal)


def test_parity_figures_recorded():
    """runs after the parity cases (file order): all of them left their figures; VSX_WRITE_PROFILES=1 writes the profile"""
    assert len(tk.FIGURES) == tk.expected_figures()
    if os.environ.get('VSX_WRITE_PROFILES') == '1':
        out = os.environ.get('VSX_PROFILE_DIR', os.path.join(ROOT, 'profiles'))
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, 'train_kernel_parity.json'), 'w') as f:
            json.dump({'device': torch.cuda.get_device_name(0),
                       'rule': 'against fp64; ideal = fp32 reference rounded to fp16: l2 <= 1.5 ideal, worst row <= 2 ideal, '
                               'max-abs <= 4 ideal, per element <= 1 fp16 ulp + 2^-10 row rms (elem_* are ratios to that bound)',
                       'cases': tk.FIGURES}, f, indent=1)
