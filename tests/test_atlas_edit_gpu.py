"""ops.atlas_edit (csrc/atlas_edit.hip, K15) and atlas.edit_atlas on the MI355X.

Kernel parity follows the rule of tests/test_atlas_gpu.py: the yardstick is the fp64 numpy restatement of
tests/atlas_edit_case.py (cell and relevance decided by the fp32 position, as in the kernel); the fp32 restatement is
measured against it on the same inputs and the kernel's max-abs error must be at most 4 x that.  Where the fp32 yardstick
is EXACTLY zero the kernel is held to one fp32 ulp of the largest output instead; that is a condition on the yardstick
being degenerate, not a tolerance.  `relevant` must be EQUAL, and the masks EQUAL to the restated scatter-max.  Only
finite coordinates are fed here: the hostile rows (NaN, infinities, 1e30) are checked on the host under the sanitizers
(tests/test_atlas_edit_cpu_check.py).  All figures are printed and collected in profiles/atlas_edit_parity.json (written
when VSX_WRITE_PROFILES=1).
"""
import json
import os

import numpy as np
import pytest
import torch

import atlas_edit_case as aec
import atlas_render_case as arc
from atlas_edit_case import F32, counted, standin
from util import ROOT

pytestmark = pytest.mark.gpu

_parity, _edit = [], []
CASES = [(n, r, c) for n in (1, 255, 256, 257, 1000) for r in (2, 16) for c in (3, 4)]
BOX_FG, BOX_BG = (0.0, 0.0, 1.0), (-0.75, -0.75, 0.5)


def _boxes(R):
    from videoswap_amd import atlas
    return atlas.texture_box(*BOX_FG, R), atlas.texture_box(*BOX_BG, R)


def _case(N, R, C):
    """finite coordinates inside and outside both boxes: fg [0, 1]^2 needs uv in [-1, 1], bg [-0.75, -0.25]^2 uv in [-0.5, 0.5]"""
    g = torch.Generator().manual_seed(1000 * N + 10 * R + C)
    uv_fg = torch.rand(N, 2, generator=g) * 2.6 - 1.3
    uv_bg = torch.rand(N, 2, generator=g) * 1.4 - 0.7
    if R == 2:                                                                 # the texture reaches px in [0, 1] only: the lower-left quarter
        uv_fg, uv_bg = uv_fg * 0.5 - 0.6, uv_bg * 0.5 - 0.3
    if N > 4:                                                                  # px == R - 1 and px == 0 exactly, and a row just outside
        top = 0.0 if R == 2 else 0.875
        uv_fg[0], uv_fg[1], uv_fg[2] = torch.tensor([top, -0.5]), torch.tensor([-1.0, -1.0]), torch.tensor([-1.001, 0.0])
    alpha = torch.rand(N, generator=g) * 0.99 + 0.001
    tex_fg, tex_bg = torch.rand(R, R, C, generator=g), torch.rand(R, R, C, generator=g)
    base_fg, base_bg = torch.rand(N, 3, generator=g), torch.rand(N, 3, generator=g)
    return uv_fg.contiguous(), uv_bg.contiguous(), alpha, tex_fg, tex_bg, base_fg, base_bg


def _bound(err32, y64):
    if err32 == 0.0:
        return float(np.spacing(F32(float(np.abs(y64).max())))), 'one fp32 ulp of the largest output (fp32 yardstick exactly 0)'
    return 4 * err32, '4 x fp32 numpy'


@pytest.mark.parametrize('N,R,C', CASES, ids=[f'N{n}-R{r}-C{c}' for n, r, c in CASES])
def test_kernel_against_fp64(N, R, C):
    from videoswap_amd import ops
    uv_fg, uv_bg, alpha, tex_fg, tex_bg, base_fg, base_bg = _case(N, R, C)
    box_fg, box_bg = _boxes(R)
    np_args = (uv_fg.numpy(), uv_bg.numpy(), alpha.numpy(), tex_fg.numpy(), box_fg, tex_bg.numpy(), box_bg,
               base_fg.numpy() if C == 4 else None, base_bg.numpy() if C == 4 else None)
    m32 = (np.zeros((R, R), F32), np.zeros((R, R), F32))
    y64 = aec.edit_rows(*np_args, dtype=np.float64)
    y32 = aec.edit_rows(*np_args, masks=m32, dtype=F32)
    masks = (torch.zeros(R, R, device='cuda'), torch.zeros(R, R, device='cuda'))
    got = ops.atlas_edit(uv_fg.cuda(), uv_bg.cuda(), alpha.cuda(), tex_fg.cuda(), box_fg, tex_bg.cuda(), box_bg,
                         base_fg=base_fg.cuda() if C == 4 else None, base_bg=base_bg.cuda() if C == 4 else None, masks=masks)
    got = [t.cpu().numpy() for t in got]
    assert np.array_equal(got[3], y64[3]) and got[3].dtype == np.uint8        # relevance: equal
    if N >= 255:                                                               # rows inside and outside each box
        assert set(np.unique(got[3] & 1)) == {0, 1} and set(np.unique(got[3] & 2)) == {0, 2}
    figures = {'N': N, 'R': R, 'C': C, 'relevant_share_fg': float((y64[3] & 1).astype(bool).mean()),
               'relevant_share_bg': float((y64[3] & 2).astype(bool).mean())}
    for k, name in enumerate(('edit', 'fg', 'bg')):
        assert got[k].shape == (N, 3) and got[k].dtype == F32 and np.isfinite(got[k]).all()
        err32 = float(np.abs(y32[k].astype(np.float64) - y64[k]).max())
        err_kernel = float(np.abs(got[k].astype(np.float64) - y64[k]).max())
        bound, rule = _bound(err32, y64[k])
        print(f'atlas_edit N={N} R={R} C={C} {name}: fp32 numpy vs fp64 {err32:.3e}, kernel vs fp64 {err_kernel:.3e}, bound {bound:.3e} '
              f'({rule}), kernel vs fp32 numpy {float(np.abs(got[k] - y32[k]).max()):.3e}')
        figures[name] = {'err_fp32_numpy': err32, 'err_kernel': err_kernel, 'bound': bound, 'rule': rule}
    _parity.append(figures)
    if N > 4:                                                                  # px == R - 1: relevant, and (C = 3) a zero colour
        assert got[3][0] & 1 and (C == 4 or not got[1][0].any()) and got[3][1] & 1 and not got[3][2] & 1 and not got[1][2].any()
    assert np.array_equal(masks[0].cpu().numpy(), m32[0]) and np.array_equal(masks[1].cpu().numpy(), m32[1])     # masks: exactly
    for name in ('edit', 'fg', 'bg'):
        assert figures[name]['err_kernel'] <= figures[name]['bound'], (name, figures[name])


def test_masks_a_thousand_rows_in_one_cell_and_untouched_by_irrelevant_rows():
    from videoswap_amd import ops
    R = 4
    box_fg, box_bg = _boxes(R)
    g = torch.Generator().manual_seed(4)
    tex_fg, tex_bg = torch.rand(R, R, 3, generator=g), torch.rand(R, R, 3, generator=g)
    # fg px = (uv * 0.5 + 0.5) * 4 within (1, 2) for uv in (-0.5, 0); bg px = (uv * 0.5 + 0.25) * 8 within (1, 2) for uv in (-0.25, 0)
    uv_fg = -0.05 - torch.rand(1000, 2, generator=g) * 0.4
    uv_bg = -0.02 - torch.rand(1000, 2, generator=g) * 0.2
    alpha = torch.rand(1000, generator=g) * 0.99 + 0.001
    start = (torch.rand(R, R, generator=g) * 0.2, (torch.rand(R, R, generator=g) > 0.5).float())      # masks the caller initialised
    masks = tuple(m.clone().cuda() for m in start)
    want = tuple(m.clone().numpy() for m in start)
    rel = aec.edit_rows(uv_fg.numpy(), uv_bg.numpy(), alpha.numpy(), tex_fg.numpy(), box_fg, tex_bg.numpy(), box_bg, masks=want)[3]
    assert (rel == 3).all()
    got_rel = ops.atlas_edit(uv_fg.cuda(), uv_bg.cuda(), alpha.cuda(), tex_fg.cuda(), box_fg, tex_bg.cuda(), box_bg, masks=masks)[3]
    assert bool((got_rel == 3).all())
    assert np.array_equal(masks[0].cpu().numpy(), want[0]) and np.array_equal(masks[1].cpu().numpy(), want[1])
    for y in (1, 2):
        for x in (1, 2):
            assert float(masks[0][y, x]) == float(alpha.max()) and float(masks[1][y, x]) == 1.0      # the true maximum of 1000 rows
    changed = (masks[0].cpu() != start[0])
    assert int(changed.sum()) == 4
    # rows outside both boxes touch nothing; only one mask given: the other layer's is simply not kept
    before = tuple(m.clone() for m in masks)
    out = ops.atlas_edit(torch.full((300, 2), 1.5, device='cuda'), torch.full((300, 2), 1.5, device='cuda'), alpha[:300].cuda(),
                         tex_fg.cuda(), box_fg, tex_bg.cuda(), box_bg, masks=masks)
    assert not bool(out[3].any()) and not bool(out[0].any()) and torch.equal(masks[0], before[0]) and torch.equal(masks[1], before[1])
    only_bg = (None, torch.zeros(R, R, device='cuda'))
    ops.atlas_edit(uv_fg.cuda(), uv_bg.cuda(), alpha.cuda(), tex_fg.cuda(), box_fg, tex_bg.cuda(), box_bg, masks=only_bg)
    assert float(only_bg[1].sum()) == 4.0


def test_rows_past_n_are_not_stored_and_n_zero_works():
    from videoswap_amd import ops
    uv_fg, uv_bg, alpha, tex_fg, tex_bg, _, _ = (t.cuda() for t in _case(600, 16, 3))
    box_fg, box_bg = _boxes(16)
    full = ops.atlas_edit(uv_fg, uv_bg, alpha, tex_fg, box_fg, tex_bg, box_bg)
    # the outputs of a 257-row call are carved out of larger buffers by the allocator; what the call returns is exactly 257 rows
    part = ops.atlas_edit(uv_fg[:257].contiguous(), uv_bg[:257].contiguous(), alpha[:257].contiguous(), tex_fg, box_fg, tex_bg, box_bg)
    for a, b in zip(part, full):
        assert a.shape[0] == 257 and torch.equal(a, b[:257])
    empty = ops.atlas_edit(uv_fg[:0].contiguous(), uv_bg[:0].contiguous(), alpha[:0].contiguous(), tex_fg, box_fg, tex_bg, box_bg)
    assert [tuple(t.shape) for t in empty] == [(0, 3), (0, 3), (0, 3), (0,)]
    # a guard behind the rows: the kernel is launched on the first 257 rows of buffers that hold 600
    from videoswap_amd import _lib
    from videoswap_amd.ops import _p, _stream
    outs = [torch.full((600, 3), -7.0, device='cuda') for _ in range(3)]
    rel = torch.full((600,), 99, dtype=torch.uint8, device='cuda')
    layer = lambda tex, box: [_p(tex), 16, 16, 3, *box, None, None, 0, 0]  # noqa: E731
    rc = _lib.load().vsx_atlas_edit_f32(_p(uv_fg), _p(uv_bg), _p(alpha), 257, *layer(tex_fg, box_fg), *layer(tex_bg, box_bg),
                                        *[_p(o) for o in outs], _p(rel), _stream())
    assert rc == 0
    for o, want in zip(outs, full):
        assert torch.equal(o[:257], want[:257]) and bool((o[257:] == -7.0).all())
    assert torch.equal(rel[:257], full[3][:257]) and bool((rel[257:] == 99).all())


def test_refusals_come_back_from_the_entry_point():
    from videoswap_amd import ops
    from videoswap_amd._lib import VsxError
    R = 16
    box_fg, box_bg = _boxes(R)
    uv, alpha = torch.zeros(8, 2, device='cuda'), torch.full((8,), 0.5, device='cuda')
    tex = torch.zeros(R * R * 3 + 4, device='cuda')
    good = tex[:R * R * 3].view(R, R, 3)
    with pytest.raises(NotImplementedError, match='channels'):
        ops.atlas_edit(uv, uv, alpha, torch.zeros(R, R, 5, device='cuda'), box_fg, good, box_bg)
    with pytest.raises(VsxError, match='not square'):
        ops.atlas_edit(uv, uv, alpha, good, box_fg, torch.zeros(R, R + 1, 3, device='cuda'), box_bg)
    with pytest.raises(VsxError, match='base colours'):
        ops.atlas_edit(uv, uv, alpha, torch.zeros(R, R, 4, device='cuda'), box_fg, good, box_bg)
    with pytest.raises(VsxError, match='mask is 8 x 8'):
        ops.atlas_edit(uv, uv, alpha, good, box_fg, good, box_bg, masks=(torch.zeros(8, 8, device='cuda'), None))
    with pytest.raises(VsxError, match='at least 2'):
        ops.atlas_edit(uv, uv, alpha, torch.zeros(1, 1, 3, device='cuda'), box_fg, good, box_bg)
    with pytest.raises(VsxError, match='16-byte aligned'):                     # a texture that starts 4 bytes into an allocation
        ops.atlas_edit(uv, uv, alpha, tex[1:R * R * 3 + 1].view(R, R, 3), box_fg, good, box_bg)
    with pytest.raises(VsxError, match='8-byte aligned'):
        ops.atlas_edit(torch.zeros(17, device='cuda')[1:].view(8, 2), uv, alpha, good, box_fg, good, box_bg)
    with pytest.raises(VsxError, match='base_fg'):
        ops.atlas_edit(uv, uv, alpha, torch.zeros(R, R, 4, device='cuda'), box_fg, good, box_bg, base_fg=torch.zeros(7, 3, device='cuda'))


@pytest.mark.parametrize('case', ['toy', 'real_widths'])
def test_edit_atlas_on_the_device_matches_the_reference_loop(case):
    """bound: 4 x the error of the fp32 stand-ins against the fp64 reference loop on the same case; pixels on which a
    run disagrees with the fp64 loop about relevance (a step) are left out of the colour comparison, at most 0.5 %"""
    from videoswap_amd import atlas
    R = 16
    if case == 'toy':
        W, H, T, frames = 48, 32, 4, [0, 1, 2, 3]
        models = arc.toy_models(arc.toy_config())
        area_fg = (0.0, 0.0, 1.0)
    else:
        W, H, T, frames = 64, 40, 2, [0, 1]
        models = arc.toy_models(arc.toy_config(real=True), grid=None, seed=7, table_range=0.05)
        area_fg = (0.25, 0.25, 0.5)
    box_fg, box_bg = atlas.texture_box(*area_fg, R), atlas.texture_box(*BOX_BG, R)
    g = torch.Generator().manual_seed(31)
    tex_fg, tex_bg = torch.rand(R, R, 3, generator=g), torch.rand(R, R, 4, generator=g)        # one replaced layer, one RGBA overlay
    want = aec.ref_edit(models, W, H, T, frames, tex_fg, box_fg, tex_bg, box_bg, torch.float64)
    with standin():
        cpu = atlas.edit_atlas(models, W, H, T, tex_fg, box_fg, tex_bg, box_bg, frames=frames, want_masks=True)
    dev = {k: m.cuda() for k, m in models.items()}
    with counted() as box:
        got = atlas.edit_atlas(dev, W, H, T, tex_fg, box_fg, tex_bg, box_bg, frames=frames, rows_per_call=W * H * 3 // 2, want_masks=True)
    chunks = -(-len(frames) * 2 // 3)
    assert box['calls'] == 5 * chunks == got['launches'] and got['edit'].is_cuda
    whole = atlas.edit_atlas(dev, W, H, T, tex_fg, box_fg, tex_bg, box_bg, frames=frames, want_masks=True)
    assert whole['launches'] == 5
    for k in ('edit', 'edited_fg', 'edited_bg', 'relevant', 'alpha', 'mask_fg', 'mask_bg'):      # chunked == unchunked on the kernels
        assert torch.equal(whole[k], got[k]), k
    rel64 = want['relevant']
    shares = {'fg': float(((rel64 & 1) != 0).float().mean()), 'bg': float(((rel64 & 2) != 0).float().mean())}
    same_cpu, same_dev = cpu['relevant'] == rel64, got['relevant'].cpu() == rel64
    left_out = {'stand_in': int((~same_cpu).sum()), 'kernel': int((~same_dev).sum()), 'pixels': rel64.numel()}
    print(f'edit {case}: relevant share fg {shares["fg"]:.3f} bg {shares["bg"]:.3f}; left out {left_out}')
    figures = {'case': case, 'res': [W, H], 'frames': len(frames), 'relevant_share': shares, 'left_out': left_out}
    assert left_out['kernel'] <= 0.005 * rel64.numel() and left_out['stand_in'] <= 0.005 * rel64.numel()
    assert 0.02 < shares['fg'] < 0.98 and 0.02 < shares['bg'] < 0.98            # both branches of both layers
    keep = same_cpu & same_dev
    for k in ('edit', 'edited_fg', 'edited_bg', 'alpha'):
        sel = keep if want[k].dim() == 3 else keep.unsqueeze(-1).expand_as(want[k])
        err_standin = float((cpu[k].double() - want[k]).abs()[sel].max())
        err_kernel = float((got[k].cpu().double() - want[k]).abs()[sel].max())
        print(f'edit {case} {k}: stand-in vs fp64 {err_standin:.3e}, kernel vs fp64 {err_kernel:.3e}')
        figures[k] = {'err_standin': err_standin, 'err_kernel': err_kernel, 'bound': 4 * err_standin}
    figures['mask_cells_differing_from_stand_in'] = {'fg': int((got['mask_fg'].cpu() != cpu['mask_fg']).sum()),
                                                     'bg': int((got['mask_bg'].cpu() != cpu['mask_bg']).sum())}
    _edit.append(figures)
    assert float(want['edit'].std()) > 0.01
    assert 0 < float(got['mask_fg'].max()) <= float(got['alpha'].max()) and set(got['mask_bg'].unique().tolist()) <= {0.0, 1.0}
    for k in ('edit', 'edited_fg', 'edited_bg', 'alpha'):
        assert figures[k]['err_kernel'] <= figures[k]['bound'], (k, figures[k])


def test_parity_figures_recorded():
    """runs after the cases above (file order): all of them left a figure; VSX_WRITE_PROFILES=1 writes the profile"""
    assert len(_parity) == len(CASES) and len(_edit) == 2
    if os.environ.get('VSX_WRITE_PROFILES') == '1':
        out = os.environ.get('VSX_PROFILE_DIR', os.path.join(ROOT, 'profiles'))
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, 'atlas_edit_parity.json'), 'w') as f:
            json.dump({'device': torch.cuda.get_device_name(0),
                       'rule': 'err_kernel <= 4 * err_fp32_numpy (max abs, vs fp64 of the same restatement; one fp32 ulp where that is 0); '
                               'relevant and masks equal; edit_atlas: 4 * the stand-in error, relevance mismatches left out (<= 0.5 %)',
                       'cases': _parity, 'edit_atlas': _edit}, f, indent=1)
