"""The hash grid, the hash-grid MLP (csrc/atlas.hip, K14) and the atlas rendering on the MI355X.

Kernel parity follows the rule of tests/test_atlas_gpu.py: the yardstick is an fp64 evaluation of the same restatement
(tests/atlas_render_case.py) on the CPU; fp32 PyTorch is measured against it on the same inputs and the kernel's max-abs
error must be at most 4 x that.  Where the fp32 yardstick is EXACTLY zero (one row at the origin: every weight is 0.5 and
every product exact), the kernel is held to one fp32 ulp of the largest output instead; that is a condition on the
yardstick being degenerate, not a tolerance.  All figures are printed and collected in
profiles/atlas_render_parity.json (written when VSX_WRITE_PROFILES=1).  tinycudann is not available: these tests pin the
kernel to the restatement, not to the library.
"""
import json
import os

import numpy as np
import pytest
import torch

import atlas_render_case as arc
from atlas_render_case import SMALL_GRID, counted, standin
from util import ROOT

pytestmark = pytest.mark.gpu

_parity, _render = [], []
_tables = {}
# (grid name, N, hidden, layers, skips, weight scale)
CASES = [('small', n, 64, 2, [], 1.0) for n in (1, 63, 64, 65, 1000)] + [('reference', 1000, 256, 8, [4, 7], s) for s in (1.0, 2.0)]
RUNS = [c + (r,) for c in CASES for r in (1e-4, 1.0)]                        # table values: tcnn's initialisation, and [-1, 1]


def _grid(name):
    from videoswap_amd.atlas import HASH_GRID
    return SMALL_GRID if name == 'small' else HASH_GRID


def _table(name, table_range):
    """one table per grid and range, shared by the cases and left unchanged"""
    from videoswap_amd.atlas import hash_grid_floats
    key = (name, table_range)
    if key not in _tables:
        g = torch.Generator().manual_seed(len(_tables) + 11)
        _tables[key] = (torch.rand(hash_grid_floats(_grid(name)), generator=g) * 2 - 1) * table_range
    return _tables[key]


def _inputs(name, N):
    """half the rows in [0, 1]^2, half in [-1, 0]^2; the first rows are 0, +-1 and lattice points k / scale_l"""
    from videoswap_amd.atlas import hash_grid_levels
    g = torch.Generator().manual_seed(N)
    x = torch.rand(N, 2, generator=g)
    x[N // 2:] -= 1.0
    special = [[0.0, 0.0], [1.0, 1.0], [-1.0, -1.0], [1.0, -1.0], [0.0, -1.0]]
    for k, lv in enumerate(hash_grid_levels(_grid(name))):
        special += [[(k + 1) / lv['scale'], -(k + 2) / lv['scale']], [-(k + 1) / lv['scale'], 1 / lv['scale']]]
    n = min(N, len(special))
    x[:n] = torch.tensor(special[:n])
    return x.contiguous()


def _bound(err_torch, y64):
    if err_torch == 0.0:                                                     # degenerate yardstick: one ulp of the largest output
        return float(np.spacing(np.float32(float(y64.abs().max())))), 'one fp32 ulp of the largest output (fp32 yardstick exactly 0)'
    return 4 * err_torch, '4 x fp32 torch'


@pytest.mark.parametrize('name,N,hidden,layers,skips,scale,table_range', RUNS,
                         ids=[f'{c[0]}-{c[1]}-x{c[5]:g}-t{c[6]:g}' for c in RUNS])
def test_kernels_against_fp64(name, N, hidden, layers, skips, scale, table_range):
    from videoswap_amd import ops
    from videoswap_amd.atlas import HashGridMLP
    grid, table, x = _grid(name), _table(name, table_range), _inputs(name, N)
    torch.manual_seed(N % 1000 + layers)
    m = HashGridMLP(2, 3, hidden_dim=hidden, mlp_layers=layers, skip_layers=skips, grid=grid)
    with torch.no_grad():
        for lin in m.hidden:
            lin.weight.mul_(scale)
            lin.bias.mul_(scale)
        m.encoder.params.copy_(table)
        e64, e32 = arc.hash_encode(x, table, grid, torch.float64), arc.hash_encode(x, table, grid, torch.float32)
        y64, y32 = arc.ref_forward(m, x, torch.float64), arc.ref_forward(m, x, torch.float32)
        m = m.cuda()
        enc = ops.hash_grid(x.cuda(), m.encoder.params.detach(), grid).cpu()
        got = m(x.cuda()).cpu()
    figures = {'grid': name, 'N': N, 'hidden': hidden, 'layers': layers, 'weight_scale': scale, 'table_range': table_range}
    for what, k, t32, t64 in (('hash_grid', enc, e32, e64), ('hash_mlp', got, y32, y64)):
        assert k.shape == t64.shape and k.dtype == torch.float32 and bool(torch.isfinite(k).all())
        err_torch = float((t32.double() - t64).abs().max())
        err_kernel = float((k.double() - t64).abs().max())
        bound, rule = _bound(err_torch, t64)
        print(f'{what} {name} N={N} scale={scale} table={table_range:g}: fp32 torch vs fp64 {err_torch:.3e}, kernel vs fp64 '
              f'{err_kernel:.3e}, bound {bound:.3e} ({rule}), max |y| {float(t64.abs().max()):.3e}')
        figures[what] = {'err_fp32_torch': err_torch, 'err_kernel': err_kernel, 'bound': bound, 'rule': rule}
    _parity.append(figures)
    for what in ('hash_grid', 'hash_mlp'):
        assert figures[what]['err_kernel'] <= figures[what]['bound'], (what, figures[what])


def test_known_answers_on_the_kernel():
    """the hand-computed answers of tests/test_atlas_render.py, on the kernel: exact"""
    from videoswap_amd import ops
    table = torch.stack((torch.arange(592.0), torch.arange(592.0) + 0.25), dim=1).reshape(-1).cuda()
    x = torch.tensor([[0.5, 0.5], [0.25, 0.375], [-0.25, -0.5]]).cuda()
    enc = ops.hash_grid(x, table, SMALL_GRID).cpu()
    assert enc[0, 0:2].tolist() == [10.0, 10.25] and enc[1, 2:4].tolist() == [43.25, 43.5] and enc[2, 6:8].tolist() == [424.25, 424.5]


def test_rows_past_n_are_not_stored():
    from videoswap_amd import ops
    table = _table('small', 1.0).cuda()
    x = _inputs('small', 128).cuda()
    full = ops.hash_grid(x, table, SMALL_GRID)
    assert torch.equal(ops.hash_grid(x[:65].contiguous(), table, SMALL_GRID), full[:65])
    assert ops.hash_grid(x[:0].contiguous(), table, SMALL_GRID).shape == (0, 8)


def test_unsupported_grids_come_back_from_the_entry_point():
    from videoswap_amd import ops
    from videoswap_amd._lib import VsxError
    from videoswap_amd.atlas import hash_grid_floats
    x = torch.zeros(4, 2, device='cuda')
    table = torch.zeros(hash_grid_floats(SMALL_GRID) + 4, device='cuda')
    packed = torch.zeros(64, device='cuda')
    for grid, xs, word in ((dict(SMALL_GRID, n_features_per_level=4), x, 'n_features_per_level'),
                           (SMALL_GRID, torch.zeros(4, 3, device='cuda'), 'input_dim'),
                           (dict(SMALL_GRID, n_levels=40), x, 'n_levels'),
                           (dict(SMALL_GRID, log2_hashmap_size=25), x, 'log2_hashmap_size')):
        with pytest.raises(NotImplementedError, match=word):
            ops.hash_grid(xs, table[:-4], grid)
        with pytest.raises(NotImplementedError, match=word):
            ops.hash_mlp(xs, table[:-4], grid, packed, 3, 64, 2)
    with pytest.raises(NotImplementedError, match='hidden_dim'):
        ops.hash_mlp(x, table[:-4], SMALL_GRID, packed, 3, 48, 2)
    with pytest.raises(VsxError, match='aligned'):                           # a table that starts 4 bytes into an allocation
        ops.hash_grid(x, table[1:-3], SMALL_GRID)
    with pytest.raises(VsxError, match='aligned'):
        ops.hash_mlp(x, table[1:-3], SMALL_GRID, packed, 3, 64, 2)
    with pytest.raises(VsxError, match='1188.*1184'):                        # a table of the wrong length is refused, not read
        ops.hash_grid(x, table, SMALL_GRID)
    with pytest.raises(VsxError, match='packed'):
        ops.hash_mlp(x, table[:-4], SMALL_GRID, packed, 3, 64, 2)


@pytest.mark.parametrize('case', ['toy', 'real_widths'])
def test_render_on_the_device_matches_the_stand_in(case):
    """bound: 4 x the error of the fp32 stand-in against the fp64 reference loop on the same case"""
    from videoswap_amd import atlas
    if case == 'toy':
        W, H, T, frames = 48, 32, 4, [0, 1, 2, 3]
        models = arc.toy_models(arc.toy_config())
    else:
        W, H, T, frames = 64, 40, 2, [0, 1]
        models = arc.toy_models(arc.toy_config(real=True), grid=None, seed=7, table_range=0.05)
    want = arc.ref_render(models, W, H, T, frames, torch.float64)
    with standin():
        cpu = atlas.render_atlas(models, W, H, T, frames=frames)
    with counted() as box:
        got = atlas.render_atlas({k: m.cuda() for k, m in models.items()}, W, H, T, frames=frames, rows_per_call=W * H * 3 // 2)
    chunks = -(-len(frames) * 2 // 3)
    assert box['calls'] == 4 * chunks == got['launches'] and got['reconstruction'].is_cuda
    figures = {'case': case, 'res': [W, H], 'frames': len(frames)}
    for k in ('reconstruction', 'alpha'):
        err_standin = float((cpu[k].double() - want[k]).abs().max())
        err_kernel = float((got[k].cpu().double() - want[k]).abs().max())
        diff = float((got[k].cpu() - cpu[k]).abs().max())
        print(f'render {case} {k}: kernel vs stand-in {diff:.3e}, stand-in vs fp64 {err_standin:.3e}, kernel vs fp64 {err_kernel:.3e}')
        figures[k] = {'kernel_vs_standin': diff, 'err_standin': err_standin, 'err_kernel': err_kernel, 'bound': 4 * err_standin}
    _render.append(figures)
    assert float(want['reconstruction'].std()) > 0.01
    for k in ('reconstruction', 'alpha'):
        assert figures[k]['err_kernel'] <= figures[k]['bound'], (k, figures[k])


def test_parity_figures_recorded():
    """runs after the cases above (file order): all of them left a figure; VSX_WRITE_PROFILES=1 writes the profile"""
    assert len(_parity) == len(RUNS) and len(_render) == 2
    if os.environ.get('VSX_WRITE_PROFILES') == '1':
        out = os.environ.get('VSX_PROFILE_DIR', os.path.join(ROOT, 'profiles'))
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, 'atlas_render_parity.json'), 'w') as f:
            json.dump({'device': torch.cuda.get_device_name(0),
                       'rule': 'err_kernel <= 4 * err_fp32_torch (max abs, vs fp64 of the same restatement); render: 4 * the stand-in error',
                       'cases': _parity, 'render': _render}, f, indent=1)
