"""Editing a video through its atlas (videoswap_amd/atlas.py edit_atlas, edit_atlas.py, ops.atlas_edit) — host side, no GPU.

`ops.atlas_edit` is replaced by the fp32 numpy restatement of tests/atlas_edit_case.py, the networks by the stand-ins of
tests/atlas_render_case.py.  The restatement itself is pinned to the reference's own get_colors through
tests/golden/atlas_edit.pt (tests/golden/make_golden_atlas_edit.py).
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import yaml

import atlas_edit_case as aec
import atlas_render_case as arc
from atlas_edit_case import F32, standin
from util import GOLDEN

ULP = 2.0 ** -24
BOX_FG, BOX_BG, R = (0.0, 0.0, 1.0), (-0.75, -0.75, 0.5), 16
TOY = dict(res_x=48, res_y=32, T=4)


def _boxes():
    from videoswap_amd import atlas
    return atlas.texture_box(*BOX_FG, R), atlas.texture_box(*BOX_BG, R)


def _textures(channels=3, seed=21):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(R, R, channels, generator=g), torch.rand(R, R, channels, generator=g)


@pytest.fixture(scope='module')
def golden():
    return torch.load(os.path.join(GOLDEN, 'atlas_edit.pt'), map_location='cpu', weights_only=True)


@pytest.fixture(scope='module')
def toy():
    return arc.toy_models(arc.toy_config())


def test_restatement_equals_the_reference_get_colors(golden):
    """The reference's get_colors computes the position in fp32 tensors and everything after it in numpy, where an int64
    corner minus an fp32 position promotes to FLOAT64: its colours are fp64 numbers formed from fp32 positions.  So
    - relevance, the positions and the masks are fp32 / integer facts and the fp32 restatement equals them BIT FOR BIT;
    - the colours and the three composed outputs equal the fp64 restatement fed the fp32 positions BIT FOR BIT;
    - the fp32 restatement's colours cannot equal fp64 numbers; they are held to 12 x 2^-24 on values in [0, 1]: per
      corner two roundings in the weight's factors, one in their product, one in texel x weight (the weights sum to 1:
      4 in all), three sums, one product with alpha, two in (1 - alpha) x colour, one final sum."""
    from videoswap_amd import atlas
    fx = golden
    assert fx['rgb_fg'].dtype == torch.float64 and fx['px_fg'].dtype == torch.float32
    box_fg, box_bg = atlas.texture_box(*fx['area_fg'], fx['R']), atlas.texture_box(*fx['area_bg'], fx['R'])
    uvf, uvb, alpha = fx['uv_fg'].numpy(), fx['uv_bg'].numpy(), fx['alpha'].numpy()
    tf, tb = fx['tex_fg'].numpy(), fx['tex_bg'].numpy()
    for layer, uv, tex, box, shift in (('fg', uvf, tf, box_fg, 0.5), ('bg', uvb, tb, box_bg, -0.5)):
        col32, rel, px, py = aec.sample(uv, tex, box, shift, F32)
        col64, rel64, _, _ = aec.sample(uv, tex, box, shift, np.float64, pos_dtype=F32)
        want_rel = fx[f'relevant_{layer}'].numpy()
        assert np.array_equal(rel, want_rel) and np.array_equal(rel64, want_rel) and 0.2 < rel.mean() < 0.9
        assert np.array_equal(px[rel], fx[f'px_{layer}'].numpy()) and np.array_equal(py[rel], fx[f'py_{layer}'].numpy())
        assert np.array_equal(col64[rel], fx[f'rgb_{layer}'].numpy())
        err = float(np.abs(col32[rel].astype(np.float64) - fx[f'rgb_{layer}'].numpy()).max())
        print(f'{layer}: fp32 restatement vs the reference colours {err:.3e}')
        assert err <= 12 * ULP
    e64, f64, b64, r64 = aec.edit_rows(uvf, uvb, alpha, tf, box_fg, tb, box_bg, dtype=np.float64, pos_dtype=F32)
    e32, f32, b32, r32 = aec.edit_rows(uvf, uvb, alpha, tf, box_fg, tb, box_bg, dtype=F32)
    want_rel = fx['relevant_fg'].numpy().astype(np.uint8) | (fx['relevant_bg'].numpy().astype(np.uint8) << 1)
    assert np.array_equal(r64, want_rel) and np.array_equal(r32, want_rel) and set(np.unique(want_rel)) == {0, 1, 2, 3}
    for name, got64, got32 in (('edit', e64, e32), ('edited_fg', f64, f32), ('edited_bg', b64, b32)):
        want = fx[name].numpy()
        assert np.array_equal(got64, want), name
        assert got32.dtype == F32 and float(np.abs(got32.astype(np.float64) - want).max()) <= 12 * ULP, name
    # the masks: rows that never share a cell, where the reference's last writer and the true maximum agree
    masks = (np.zeros((fx['R'], fx['R']), F32), np.zeros((fx['R'], fx['R']), F32))
    _, _, _, rel = aec.edit_rows(fx['mask_uv_fg'].numpy(), fx['mask_uv_bg'].numpy(), fx['mask_alpha'].numpy(), tf, box_fg, tb,
                                 box_bg, masks=masks, dtype=F32)
    assert (rel == 3).all() and fx['mask_fg'].dtype == torch.float64
    assert np.array_equal(masks[0].astype(np.float64), fx['mask_fg'].numpy()) and np.array_equal(masks[1].astype(np.float64), fx['mask_bg'].numpy())
    assert int((masks[0] > 0).sum()) == 4 * fx['mask_alpha'].numel() == int(masks[1].sum())


def test_recorded_golden_is_what_the_reference_gives_now(golden):
    """when the reference's tree is readable the generator is run again: the committed file is its output"""
    import importlib.util
    spec = importlib.util.spec_from_file_location('make_golden_atlas_edit', os.path.join(GOLDEN, 'make_golden_atlas_edit.py'))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert sorted(k for k in golden) and golden['uv_fg'].shape == (gen.N_ROWS, 2) and golden['mask_alpha'].numel() <= 16
    if gen.reference_available():
        fresh = gen.generate()
        assert sorted(fresh) == sorted(golden)
        for k, v in fresh.items():
            assert torch.equal(v, golden[k]) if torch.is_tensor(v) else v == golden[k], k


def test_known_answers():
    """Bilinear interpolation reproduces an affine texture a x + b y + c: the colour at (px, py) is a px + b py + c.
    Compared in fp64 under the fp32 rule (the position is the fp32 one); the texture is stored in fp32, so each texel is
    within 2^-25 of the affine value and, the weights summing to 1, so is the colour: bound 2^-24."""
    from videoswap_amd import atlas, ops
    box_fg, box_bg = _boxes()
    a, b, c = np.array([0.03, 0.01, 0.0]), np.array([0.02, 0.04, 0.05]), np.array([0.1, 0.2, 0.0])
    yy, xx = np.meshgrid(np.arange(R), np.arange(R), indexing='ij')
    tex = (xx[..., None] * a + yy[..., None] * b + c).astype(F32)
    g = torch.Generator().manual_seed(3)
    uv_fg = (torch.rand(500, 2, generator=g) * 2 - 1) * (15 / 16)            # fg: px = (uv * 0.5 + 0.5) * 16 within [0.5, 15.5)
    uv_fg[0] = torch.tensor([0.875, 0.0])                                      # px == R - 1 exactly
    uv_fg[1] = torch.tensor([-1.0, -1.0])                                      # px == 0 exactly
    uv_bg = torch.rand(500, 2, generator=g) - 0.5                              # bg: px = (uv * 0.5 - 0.5 + 0.75) * 32 within [0, 16)
    alpha = torch.rand(500, generator=g) * 0.99 + 0.001
    for layer, uv, box, shift in (('fg', uv_fg, box_fg, 0.5), ('bg', uv_bg, box_bg, -0.5)):
        col, rel, px, py = aec.sample(uv.numpy(), tex, box, shift, np.float64, pos_dtype=F32)
        inner = rel & (px < R - 1) & (py < R - 1)
        want = px.astype(np.float64)[:, None] * a + py.astype(np.float64)[:, None] * b + c
        assert inner.sum() > 200 and float(np.abs(col - want)[inner].max()) <= ULP
    with standin():
        edit, fg, bg, rel = ops.atlas_edit(uv_fg, uv_bg, alpha, torch.from_numpy(tex), box_fg, torch.from_numpy(tex), box_bg)
    assert edit.shape == fg.shape == bg.shape == (500, 3) and rel.dtype == torch.uint8 and rel.shape == (500,)
    _, relb, pxb, pyb = aec.sample(uv_bg.numpy(), tex, box_bg, -0.5, F32)
    inner = torch.from_numpy(relb & (pxb < R - 1) & (pyb < R - 1))
    want_bg = torch.from_numpy(pxb.astype(np.float64)[:, None] * a + pyb.astype(np.float64)[:, None] * b + c)
    assert float((bg.double() - want_bg).abs()[inner].max()) <= 12 * ULP      # the fp32 op, same bound as against the golden
    # px == R - 1: x0 == x1 after the clip, both weights along x vanish: a relevant row with a zero colour
    assert int(rel[0]) & 1 and fg[0].tolist() == [0.0, 0.0, 0.0]
    assert int(rel[1]) & 1 and float((fg[1].double() - torch.from_numpy(c) * float(alpha[1])).abs().max()) <= 12 * ULP


def test_rows_outside_each_edge_are_not_relevant_and_zero():
    from videoswap_amd import ops
    box_fg, box_bg = _boxes()
    tex_fg, tex_bg = _textures()
    inside = 0.1
    # fg px = (uv * 0.5 + 0.5) * 16: uv < -1 is left / above, uv > 0.875 has ceil(px) == 16
    rows = [[-1.01, inside], [0.8751, inside], [inside, -1.01], [inside, 0.8751], [inside, inside]]
    uv_fg = torch.tensor(rows)
    # bg px = (uv * 0.5 + 0.25) * 32: uv < -0.5 is outside, uv > 0.4375 has ceil(px) == 16
    uv_bg = torch.tensor([[-0.51, inside], [0.4376, inside], [inside, -0.51], [inside, 0.4376], [inside, inside]])
    alpha = torch.full((5,), 0.5)
    masks = (torch.zeros(R, R), torch.zeros(R, R))
    with standin():
        edit, fg, bg, rel = ops.atlas_edit(uv_fg, uv_bg, alpha, tex_fg, box_fg, tex_bg, box_bg, masks=masks)
    assert rel.tolist() == [0, 0, 0, 0, 3]
    assert float(edit[:4].abs().max()) == 0 and float(fg[:4].abs().max()) == 0 and float(bg[:4].abs().max()) == 0
    assert float(fg[4].min()) > 0 and float(bg[4].min()) > 0 and torch.allclose(edit[4], fg[4] + bg[4] * 0.5)
    assert int((masks[0] > 0).sum()) == 4 == int(masks[1].sum()) and float(masks[0].max()) == 0.5   # the one relevant row only


def test_rgba_overlay_alpha_zero_is_the_base_alpha_one_the_texture():
    from videoswap_amd import ops
    box_fg, box_bg = _boxes()
    rgb_fg, rgb_bg = _textures()
    g = torch.Generator().manual_seed(8)
    uv_fg, uv_bg = torch.rand(64, 2, generator=g) * 1.6 - 0.8, torch.rand(64, 2, generator=g) * 0.8 - 0.4     # all inside
    alpha = torch.rand(64, generator=g) * 0.99 + 0.001
    base_fg, base_bg = torch.rand(64, 3, generator=g), torch.rand(64, 3, generator=g)
    with standin():
        plain = ops.atlas_edit(uv_fg, uv_bg, alpha, rgb_fg, box_fg, rgb_bg, box_bg)
        for a in (0.0, 1.0):
            over_fg = torch.cat((rgb_fg, torch.full((R, R, 1), a)), dim=2)
            over_bg = torch.cat((rgb_bg, torch.full((R, R, 1), a)), dim=2)
            edit, fg, bg, rel = ops.atlas_edit(uv_fg, uv_bg, alpha, over_fg, box_fg, over_bg, box_bg, base_fg=base_fg, base_bg=base_bg)
            assert (rel == 3).all()
            if a == 0.0:                                                       # colour * 0 + base * 1: exactly the base
                assert torch.equal(bg, base_bg) and torch.equal(fg, base_fg * alpha.unsqueeze(1))
            else:       # the overlay's alpha interpolates to 1 within 7 x 2^-24 (four products, three sums); colour and base are
                        # below 1, and the blend adds two roundings: 2 x 7 + 2 = 16
                assert float((bg - plain[2]).abs().max()) <= 16 * ULP and float((fg - plain[1]).abs().max()) <= 16 * ULP
        # a mixed pair: only the RGBA layer needs its base
        edit, fg, bg, rel = ops.atlas_edit(uv_fg, uv_bg, alpha, over_fg, box_fg, rgb_bg, box_bg, base_fg=base_fg)
        assert torch.equal(bg, plain[2])


def test_edit_atlas_matches_the_reference_loop_in_fp64(toy):
    """Bound.  uv_fg / uv_bg of the fp32 networks are within 1e-5 of fp64 (tests/test_atlas_render.py holds them to that);
    a texel position is uv * 0.5 * pixel_size with pixel_size 16 (fg) and 32 (bg): at most 1.6e-4 texel.  A bilinear
    surface over texels in [0, 1] has a slope of at most 2 per texel (both axes), so the colour moves by at most 3.2e-4,
    and alpha (within 1e-5) scales colours below 1: 3.5e-4 in all.  Relevance is a step: pixels on which the two
    precisions disagree are left out, and there may be at most 0.5 % of them."""
    from videoswap_amd import atlas
    box_fg, box_bg = _boxes()
    tex_fg, tex_bg = _textures()
    frames = [0, 1, 2, 3]
    with standin():
        got = atlas.edit_atlas(toy, TOY['res_x'], TOY['res_y'], TOY['T'], tex_fg, box_fg, tex_bg, box_bg, frames=frames, want_masks=True)
    want = aec.ref_edit(toy, TOY['res_x'], TOY['res_y'], TOY['T'], frames, tex_fg, box_fg, tex_bg, box_bg, torch.float64)
    assert got['edit'].shape == got['edited_fg'].shape == got['edited_bg'].shape == (4, 32, 48, 3)
    assert got['relevant'].shape == got['alpha'].shape == (4, 32, 48) and got['relevant'].dtype == torch.uint8
    same = got['relevant'] == want['relevant']
    share_fg, share_bg = float(((want['relevant'] & 1) != 0).float().mean()), float(((want['relevant'] & 2) != 0).float().mean())
    print(f'relevant share fg {share_fg:.3f} bg {share_bg:.3f}; pixels left out {int((~same).sum())} of {same.numel()}')
    assert float((~same).float().mean()) <= 0.005 and 0.02 < share_fg < 0.98 and 0.02 < share_bg < 0.98
    for k in ('edit', 'edited_fg', 'edited_bg', 'alpha'):
        diff = (got[k].double() - want[k]).abs()
        err = float((diff[same] if diff.dim() == 3 else diff[same.unsqueeze(-1).expand_as(diff)]).max())
        print(f'edit_atlas vs fp64 reference loop, {k}: {err:.3e}')
        assert err <= (1e-5 if k == 'alpha' else 3.5e-4), (k, err)
    assert float(want['edit'].std()) > 0.02
    # the masks against the same loop in fp32 (the stand-ins compute what it computes): exactly the scatter-max
    want32 = aec.ref_edit(toy, TOY['res_x'], TOY['res_y'], TOY['T'], frames, tex_fg, box_fg, tex_bg, box_bg, torch.float32)
    assert torch.equal(got['relevant'], want32['relevant'])
    assert torch.equal(got['mask_fg'], want32['mask_fg']) and torch.equal(got['mask_bg'], want32['mask_bg'])
    assert 0 < float(got['mask_fg'].max()) <= float(got['alpha'].max()) and set(got['mask_bg'].unique().tolist()) == {0.0, 1.0}
    # a subset of frames is the same pixels
    with standin():
        sub = atlas.edit_atlas(toy, TOY['res_x'], TOY['res_y'], TOY['T'], tex_fg, box_fg, tex_bg, box_bg, frames=[3, 1])
    assert torch.equal(sub['edit'], got['edit'][[3, 1]]) and sub['mask_fg'] is None and sub['mask_bg'] is None


def test_launch_counts_are_four_and_five_per_chunk(toy):
    from videoswap_amd import atlas
    box_fg, box_bg = _boxes()
    n = TOY['res_x'] * TOY['res_y']
    for channels, per_chunk in ((3, 4), (4, 5)):
        tex_fg, tex_bg = _textures(channels)
        for frames, rows, chunks in (([0], 1 << 20, 1), ([0, 1, 2], 1 << 20, 1), ([0, 1, 2], 2 * n, 2), ([0, 1, 2], 1000, 5)):
            with standin() as (c, h, e):
                out = atlas.edit_atlas(toy, TOY['res_x'], TOY['res_y'], TOY['T'], tex_fg, box_fg, tex_bg, box_bg, frames=frames,
                                       rows_per_call=rows)
            assert c.calls == 3 * chunks and e.calls == chunks and h.calls == (chunks if channels == 4 else 0)
            assert out['launches'] == per_chunk * chunks and sum(e.rows) == len(frames) * n
            if channels == 4:
                assert sum(h.rows) == 2 * len(frames) * n                      # both base colours from ONE F_Atlas launch per chunk
    # one RGBA layer is enough for the fifth launch
    with standin() as (c, h, e):
        out = atlas.edit_atlas(toy, TOY['res_x'], TOY['res_y'], TOY['T'], _textures(4)[0], box_fg, _textures(3)[1], box_bg, frames=[0])
    assert out['launches'] == 5 and h.calls == 1


class _Rowwise(torch.nn.Module):
    """a stand-in network of single IEEE operations per element (products, sums, a clamp): a row's output cannot depend on
    the rows it is batched with, which a BLAS-backed nn.Linear on the CPU does not promise"""

    def __init__(self, kind, gain):
        super().__init__()
        self.kind, self.gain = kind, torch.nn.Parameter(torch.tensor(gain))

    def forward(self, x):
        g = self.gain.detach()
        if self.kind == 'mapping':
            y = x[:, :2] * g + x[:, 2:3] * 0.3
        elif self.kind == 'alpha':
            y = x[:, :1] * g - x[:, 1:2] * 0.5
        else:
            y = torch.cat((x, x[:, :1] * x[:, 1:2]), dim=1) * g
        return y.clamp(-1, 1)


def test_chunked_equals_unchunked():
    """chunks cut across frame borders: the same rows in the same order, and the masks collected over all chunks"""
    from videoswap_amd import atlas
    box_fg, box_bg = _boxes()
    models = {'FG_UV_Mapping': _Rowwise('mapping', 1.1), 'BG_UV_Mapping': _Rowwise('mapping', -0.6), 'F_Alpha': _Rowwise('alpha', 0.9),
              'F_Atlas': _Rowwise('atlas', 0.8)}
    n = TOY['res_x'] * TOY['res_y']
    for channels in (3, 4):
        tex_fg, tex_bg = _textures(channels)
        outs = []
        for rows in (1 << 20, 2 * n, 1000, n - 7):
            with standin():
                outs.append(atlas.edit_atlas(models, TOY['res_x'], TOY['res_y'], TOY['T'], tex_fg, box_fg, tex_bg, box_bg, frames=[0, 3, 1],
                                             rows_per_call=rows, want_masks=True))
        rel = outs[0]['relevant']
        assert 0.05 < float(((rel & 1) != 0).float().mean()) < 0.95 and 0.05 < float(((rel & 2) != 0).float().mean()) < 0.95
        assert float(outs[0]['mask_fg'].max()) > 0 and float(outs[0]['mask_bg'].max()) == 1
        for other in outs[1:]:
            for k in ('edit', 'edited_fg', 'edited_bg', 'relevant', 'alpha', 'mask_fg', 'mask_bg'):
                assert torch.equal(other[k], outs[0][k]), (channels, k)


def test_texture_box_forms_the_pixel_size_in_fp32_tensors():
    from videoswap_amd import atlas
    assert atlas.texture_box(0, 0, 1, 1000) == (0.0, 0.0, 1000.0)
    minx, miny, edge = -0.73, -0.81, 0.37
    mx, e = torch.tensor(minx), torch.tensor(edge)
    want = 1000 / ((mx + e) - mx)                                              # evaluate.py:65 on the arguments of :224
    got = atlas.texture_box(minx, miny, edge, 1000)
    assert got == (float(mx), float(torch.tensor(miny)), float(want)) and all(float(F32(v)) == v for v in got)
    assert got[2] != float(F32(1000 / edge)) and got[2] != float(F32(1000 / float(e)))     # not the double quotient rounded


def test_checkerboard_composites(toy):
    from videoswap_amd import atlas
    board = atlas.checkerboard(500)
    assert board.shape == (500, 500, 3) and set(board.unique().tolist()) == {0.0, 1.0}
    assert float(board[0, 0, 0]) == 1 and float(board[0, 50, 0]) == 0 and float(board[50, 50, 0]) == 1 and float(board[499, 499, 0]) == 1
    assert abs(float(board.mean()) - 0.5) < 1e-6
    with standin() as (c, h, e):
        out = atlas.checkerboard_videos(toy, TOY['res_x'], TOY['res_y'], TOY['T'], (0.1, 0.2, 0.6), (-0.75, -0.75, 0.5), frames=[0, 2],
                                        resolution=40, squares=4)
        plain = atlas.edit_atlas(toy, TOY['res_x'], TOY['res_y'], TOY['T'], out['texture_fg'], atlas.texture_box(0.1, 0.2, 0.6, 40),
                                 out['texture_bg'], atlas.texture_box(-0.75, -0.75, 0.5, 40), frames=[0, 2])
    assert out['launches'] == 4 + 2 and h.calls == 2 and out['texture_fg'].shape == (40, 40, 3)
    rel = plain['relevant']
    assert out['checkerboard_fg'].shape == out['checkerboard_bg'].shape == (2, 32, 48, 3)
    assert bool((out['checkerboard_fg'][(rel & 1) == 0] == 0.5).all()) and bool((out['checkerboard_bg'][(rel & 2) == 0] == 0.5).all())
    on = (rel & 1) != 0
    assert torch.equal(out['checkerboard_fg'][on], (0.5 * (1 - plain['alpha']).unsqueeze(-1) + plain['edited_fg'])[on])
    assert torch.equal(out['checkerboard_bg'][(rel & 2) != 0], plain['edited_bg'][(rel & 2) != 0])
    assert 0 < int(on.sum()) < on.numel()


def test_command_round_trip_render_then_edit(tmp_path):
    """render_atlas.run -> edit_atlas.run on its output directory.  Untouched textures: every file is written.  Fully
    transparent RGBA overlays: the atlas's own colours come through, so `edit` IS the reconstruction wherever both layers
    reach their texture (five launches per chunk)."""
    from PIL import Image

    from videoswap_amd import atlas, edit_atlas, render_atlas
    config = arc.toy_config()
    models = arc.toy_models(config, grid=None, seed=3, table_range=0.5)      # the reference's own grid, as a checkpoint has it
    W, H, T = 40, 24, 3
    cfg_path, ckpt_path = str(tmp_path / 'atlas.yml'), str(tmp_path / 'models.pth')
    with open(cfg_path, 'w') as f:
        yaml.safe_dump({'name': 'toy', 'datasets': {'res_x': W, 'res_y': H, 'max_frames': T, 'frame_path': str(tmp_path / 'none')},
                        'models': config}, f)
    torch.save({k: m.state_dict() for k, m in models.items()}, ckpt_path)
    rdir, save = str(tmp_path / 'render'), str(tmp_path / 'edit')
    common = ['--atlas_config_path', cfg_path, '--atlas_model_path', ckpt_path, '--num_frames', str(T)]
    with standin():
        render_atlas.run(render_atlas.parse_args(common + ['--save_dir', rdir, '--texture_resolution', '32']), device=torch.device('cpu'))
        args = edit_atlas.parse_args(common + ['--save_dir', save, '--render_dir', rdir, '--frames', '0,2', '--checkerboard', '--write_masks'])
        assert args.frames == [0, 2]
        summary = edit_atlas.run(args, device=torch.device('cpu'))
        first = atlas.render_atlas(atlas.load_atlas_models(cfg_path, ckpt_path, names=atlas.RENDER_MODEL_NAMES), W, H, T, frames=[0, 2])
    assert sorted(os.listdir(save)) == ['checkerboard_bg', 'checkerboard_fg', 'edit', 'edited_bg', 'edited_fg', 'summary.json',
                                        'texture_edit1.png', 'texture_edit2.png']
    for sub in ('edit', 'edited_fg', 'edited_bg', 'checkerboard_fg', 'checkerboard_bg'):
        assert sorted(os.listdir(os.path.join(save, sub))) == ['00000.png', '00002.png']
        assert Image.open(os.path.join(save, sub, '00002.png')).size == (W, H)
    assert Image.open(os.path.join(save, 'texture_edit1.png')).size == (32, 32) == Image.open(os.path.join(save, 'texture_edit2.png')).size
    with open(os.path.join(save, 'summary.json')) as f:
        on_disk = json.load(f)
    assert on_disk == json.loads(json.dumps(summary))
    assert on_disk['edit_launches'] == 4 and on_disk['launches'] == 4 + 6 and on_disk['frames'] == [0, 2]
    assert on_disk['texture_fg'] == {'resolution': 32, 'channels': 3, 'box': [0.0, 0.0, 32.0]}
    with open(os.path.join(rdir, 'summary.json')) as f:
        area = json.load(f)['background_box']
    assert on_disk['texture_bg']['box'] == list(atlas.texture_box(area['minx'], area['miny'], area['edge_size'], 32))
    assert 0 < on_disk['relevant_share_fg'] <= 1 and 0 < on_disk['relevant_share_bg'] <= 1
    # transparent overlays on both layers
    for name in ('fg', 'bg'):
        Image.fromarray(np.zeros((32, 32, 4), np.uint8)).save(str(tmp_path / f'clear_{name}.png'))
    save2 = str(tmp_path / 'edit2')
    with standin():
        s2 = edit_atlas.run(edit_atlas.parse_args(common + ['--save_dir', save2, '--render_dir', rdir, '--frames', '0,2', '--edit_fg',
                                                            str(tmp_path / 'clear_fg.png'), '--edit_bg', str(tmp_path / 'clear_bg.png')]),
                            device=torch.device('cpu'))
        out = atlas.edit_atlas(atlas.load_atlas_models(cfg_path, ckpt_path, names=atlas.RENDER_MODEL_NAMES), W, H, T, torch.zeros(32, 32, 4),
                               atlas.texture_box(0, 0, 1, 32), torch.zeros(32, 32, 4),
                               atlas.texture_box(area['minx'], area['miny'], area['edge_size'], 32), frames=[0, 2])
    assert s2['edit_launches'] == 5 and s2['texture_fg']['channels'] == 4 and sorted(os.listdir(save2)) == ['edit', 'edited_bg', 'edited_fg', 'summary.json']
    both = out['relevant'] == 3
    assert float(both.float().mean()) > 0.05
    assert float((out['edit'] - first['reconstruction'])[both].abs().max()) <= 4 * ULP
    back = np.asarray(Image.open(os.path.join(save2, 'edit', '00002.png')), dtype=np.float32) / 255
    assert float(np.abs(back - out['edit'][1].clamp(0, 1).numpy()).max()) <= 0.5 / 255 + 1e-6
    with pytest.raises(SystemExit):
        edit_atlas.parse_args(common + ['--save_dir', save, '--render_dir', rdir, '--frames', 'a,b'])


def test_refusals_of_the_op_and_of_the_entry_point():
    from videoswap_amd import _lib, atlas, ops
    from videoswap_amd._lib import VsxError
    box_fg, box_bg = _boxes()
    tex_fg, tex_bg = _textures()
    uv, alpha = torch.zeros(4, 2), torch.full((4,), 0.5)
    with standin():
        with pytest.raises(NotImplementedError, match='channels'):
            ops.atlas_edit(uv, uv, alpha, torch.zeros(R, R, 5), box_fg, tex_bg, box_bg)
        with pytest.raises(VsxError, match='square'):
            ops.atlas_edit(uv, uv, alpha, torch.zeros(R, R + 1, 3), box_fg, tex_bg, box_bg)
        with pytest.raises(VsxError, match='base'):
            ops.atlas_edit(uv, uv, alpha, torch.zeros(R, R, 4), box_fg, tex_bg, box_bg)
        with pytest.raises(VsxError, match='mask'):
            ops.atlas_edit(uv, uv, alpha, tex_fg, box_fg, tex_bg, box_bg, masks=(torch.zeros(R, R), torch.zeros(8, 8)))
        with pytest.raises(VsxError, match='at least 2'):
            ops.atlas_edit(uv, uv, alpha, torch.zeros(1, 1, 3), box_fg, tex_bg, box_bg)
        with pytest.raises(VsxError):
            ops.atlas_edit(uv.double(), uv, alpha, tex_fg, box_fg, tex_bg, box_bg)
        with pytest.raises(NotImplementedError, match='tex_fg'):
            atlas.edit_atlas({k: torch.nn.Linear(1, 1) for k in ('FG_UV_Mapping', 'BG_UV_Mapping', 'F_Atlas', 'F_Alpha')}, 4, 4, 1,
                             torch.zeros(R, R, 2), box_fg, tex_bg, box_bg)
    with pytest.raises(VsxError, match='GPU tensor'):                          # the real op has no CPU implementation
        ops.atlas_edit(uv, uv, alpha, tex_fg, box_fg, tex_bg, box_bg)
    # the entry point itself (host code of the library: every refusal comes back before anything is read or launched)
    lib = _lib.load()
    buf = np.zeros(64 + 4, np.float32)
    base = buf.ctypes.data + (-buf.ctypes.data) % 16                           # a 16-byte aligned address inside buf
    out = np.zeros(16, np.float32).ctypes.data

    def call(h=2, w=2, c=3, tex=base, base_rows=None, mask=None, mh=0, mw=0, n=0):
        layer = [ctypes.c_void_p(tex), h, w, c, 0.0, 0.0, 2.0, base_rows, mask, mh, mw]
        good = [ctypes.c_void_p(base), 2, 2, 3, 0.0, 0.0, 2.0, None, None, 0, 0]
        return lib.vsx_atlas_edit_f32(out, out, out, n, *layer, *good, out, out, out, out, None)

    assert call() == 0 and call(c=4, base_rows=out, mask=out, mh=2, mw=2) == 0                  # N = 0 works
    for kwargs, code, word in ((dict(c=5), _lib.VSX_E_UNSUPPORTED, 'channels'), (dict(c=1), _lib.VSX_E_UNSUPPORTED, 'channels'),
                               (dict(h=2, w=3), -1, 'not square'), (dict(h=1, w=1), -1, 'at least 2'),
                               (dict(h=26755, w=26755), -1, '32-bit'), (dict(c=4), -1, 'base colours'),
                               (dict(mask=out, mh=2, mw=4), -1, 'mask is 2 x 4'), (dict(tex=base + 4), -1, '16-byte aligned')):
        assert call(**kwargs) == code, kwargs
        assert word in lib.vsx_last_error().decode(), (kwargs, lib.vsx_last_error())
    assert _lib.VSX_ABI_VERSION == lib.vsx_abi_version() >= 15       # (the entry point is ABI 15's)
