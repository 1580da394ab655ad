"""Rendering a trained atlas (videoswap_amd/atlas.py, render_atlas.py) — host side, no GPU.

`ops.hash_mlp`, `ops.hash_grid` and `ops.coord_mlp` are replaced by the CPU stand-ins of tests/atlas_render_case.py and
tests/atlas_case.py.  tinycudann is not available, so nothing here compares with the real library: the level tables and
the known answers below pin the RESTATEMENT of include/vsx.h K14, computed by hand from the published algorithm.
"""
import json
import math
import os

import numpy as np
import pytest
import torch
import yaml

import atlas_render_case as arc
from atlas_render_case import SMALL_GRID, standin


def test_level_table_of_the_reference_configuration():
    from videoswap_amd.atlas import HASH_GRID, hash_grid_floats, hash_grid_levels
    assert HASH_GRID == dict(n_levels=16, n_features_per_level=2, log2_hashmap_size=19, base_resolution=16, per_level_scale=1.38)
    lv = hash_grid_levels()
    assert [v['res'] for v in lv] == [16, 23, 31, 43, 59, 81, 111, 153, 211, 291, 401, 554, 764, 1054, 1454, 2006]
    assert [v['hashed'] for v in lv] == [False] * 12 + [True] * 4
    assert all(v['entries'] == (v['res'] ** 2 + 7) // 8 * 8 for v in lv[:12]) and all(v['entries'] == 1 << 19 for v in lv[12:])
    assert [v['offset'] for v in lv] == [sum(u['entries'] for u in lv[:i]) for i in range(16)]
    assert sum(v['entries'] for v in lv) == 2743512 and hash_grid_floats() == 5487024


def test_level_table_of_the_small_configuration():
    from videoswap_amd.atlas import hash_grid_floats, hash_grid_levels
    lv = hash_grid_levels(SMALL_GRID)
    assert [v['scale'] for v in lv] == [3.0, 7.0, 15.0, 31.0]
    assert [v['res'] for v in lv] == [4, 8, 16, 32]
    assert [v['entries'] for v in lv] == [16, 64, 256, 256]
    assert [v['hashed'] for v in lv] == [False, False, False, True]          # level 2: res^2 == entries stays dense
    assert sum(v['entries'] for v in lv) == 592 and hash_grid_floats(SMALL_GRID) == 1184


def test_level_table_equals_the_library():
    """the pure-Python table and the one the entry points derive (csrc/atlas.hip hg_geometry) are the same numbers,
    the fp32 scale included (host code of the library: no GPU needed)"""
    from videoswap_amd import _lib
    from videoswap_amd.atlas import HASH_GRID, hash_grid_levels
    lib = _lib.load()
    for cfg in (HASH_GRID, SMALL_GRID, dict(SMALL_GRID, n_levels=32, log2_hashmap_size=24, base_resolution=7, per_level_scale=1.51)):
        L = cfg['n_levels']
        scale = np.zeros(L, np.float32)
        ints = [np.zeros(L, np.uint32) for _ in range(4)]
        floats = lib.vsx_hash_grid_geometry(L, 2, cfg['log2_hashmap_size'], cfg['base_resolution'], cfg['per_level_scale'],
                                            scale.ctypes.data, *[a.ctypes.data for a in ints])
        lv = hash_grid_levels(cfg)
        assert floats == 2 * sum(v['entries'] for v in lv)
        assert [np.float32(v['scale']) for v in lv] == list(scale)
        for key, arr in zip(('res', 'entries', 'offset', 'hashed'), ints):
            assert [int(v[key]) for v in lv] == [int(a) for a in arr], key
    assert lib.vsx_hash_grid_geometry(4, 4, 8, 4, 2.0, None, None, None, None, None) == _lib.VSX_E_UNSUPPORTED
    assert b'n_features_per_level' in lib.vsx_last_error()


def _by_hand(x0, x1, lv):
    """one level of the grid on Python scalars, uint32 arithmetic spelled out; table[e] = (e, e + 0.25)"""
    M = 0xffffffff
    p0, p1 = lv['scale'] * x0 + 0.5, lv['scale'] * x1 + 0.5
    g0, g1 = math.floor(p0) & M, math.floor(p1) & M                            # Python's & on a negative int is two's complement
    w0, w1 = p0 - math.floor(p0), p1 - math.floor(p1)
    f = 0.0
    for c in range(4):
        c0, c1 = (g0 + (c & 1)) & M, (g1 + (c >> 1)) & M
        idx, stride = c0, lv['res']
        if stride <= lv['entries']:
            idx, stride = (idx + c1 * stride) & M, (stride * lv['res']) & M
        if lv['entries'] < stride:
            idx = c0 ^ ((c1 * 2654435761) & M)
        f += (w0 if c & 1 else 1 - w0) * (w1 if c >> 1 else 1 - w1) * (idx % lv['entries'] + lv['offset'])
    return f


def test_known_answers_on_the_small_grid():
    """Table entry e holds (e, e + 0.25).  Worked by hand (offsets 0, 16, 80, 336):
    (0.5, 0.5), level 0 (scale 3, res 4): pos (2, 2), weights (0, 0): the single corner 2 + 2 * 4 = entry 10.
    (0.25, 0.375), level 1 (scale 7, res 8): pos (2.25, 3.125): entries 16 + {26, 27, 34, 35} with the weights
      {.65625, .21875, .09375, .03125} -> 43.25.
    (-0.25, -0.5), level 3 (scale 31, hashed, 256 entries): pos (-7.25, -15): g = (2^32 - 8, 2^32 - 15), weights (0.75, 0):
      the low bytes are 0xF8 / 0xF9 and 0xF1; 0xF1 * 0xB1 (low byte of 2654435761) = 0xA1 mod 256; 0xF8 ^ 0xA1 = 89 and
      0xF9 ^ 0xA1 = 88 -> 0.25 * (336 + 89) + 0.75 * (336 + 88) = 424.25."""
    from videoswap_amd import ops
    from videoswap_amd.atlas import hash_grid_levels
    table = torch.stack((torch.arange(592.0), torch.arange(592.0) + 0.25), dim=1).reshape(-1)
    x = torch.tensor([[0.5, 0.5], [0.25, 0.375], [-0.25, -0.5]])
    with standin():
        enc = ops.hash_grid(x, table, SMALL_GRID)
    assert enc.shape == (3, 8) and enc.dtype == torch.float32
    assert enc[0, 0:2].tolist() == [10.0, 10.25]
    assert enc[1, 2:4].tolist() == [43.25, 43.5]
    assert enc[2, 6:8].tolist() == [424.25, 424.5]
    lv = hash_grid_levels(SMALL_GRID)
    assert (_by_hand(0.5, 0.5, lv[0]), _by_hand(0.25, 0.375, lv[1]), _by_hand(-0.25, -0.5, lv[3])) == (10.0, 43.25, 424.25)
    for q in range(3):                                                         # every level of every query, both features
        for l in range(4):
            want = _by_hand(float(x[q, 0]), float(x[q, 1]), lv[l])
            assert abs(float(enc[q, 2 * l]) - want) <= 1e-4 * max(1.0, want), (q, l)
            assert abs(float(enc[q, 2 * l + 1]) - want - 0.25) <= 1e-4 * max(1.0, want), (q, l)


def test_state_dict_round_trip_with_the_reference_key_names():
    from videoswap_amd.atlas import HashGridMLP
    kw = arc.toy_config()['F_Atlas']
    m = HashGridMLP(**kw, grid=SMALL_GRID)
    assert sorted(m.state_dict()) == sorted(['encoder.params'] + [f'hidden.{i}.{p}' for i in range(4) for p in ('weight', 'bias')])
    assert m.state_dict()['encoder.params'].shape == (1184,) and float(m.encoder.params.detach().abs().max()) <= 1e-4
    assert m.hidden[0].in_features == 8 and m.hidden[2].in_features == 64 + 8
    other = HashGridMLP(**kw, grid=SMALL_GRID)
    other.load_state_dict({k: v.clone() for k, v in m.state_dict().items()})
    x = torch.rand(50, 2) * 2 - 1
    with standin() as (_, h), torch.no_grad():
        a, b = m(x), other(x)
        assert h.calls == 2 and torch.equal(a, b)
        want = arc.ref_forward(m, x, torch.float64)
    assert float((a.double() - want).abs().max()) <= 1e-5
    full = HashGridMLP(2, 3, hidden_dim=32, mlp_layers=2)                      # the reference's grid
    assert full.encoder.params.numel() == 5487024 and full.hidden[0].in_features == 32
    p = full.packed()
    assert full.packed() is p


def test_wrong_table_length_names_both_numbers():
    from videoswap_amd.atlas import HashGridMLP
    from videoswap_amd.formats import FormatError
    m = HashGridMLP(**arc.toy_config()['F_Atlas'], grid=SMALL_GRID)
    sd = dict(m.state_dict(), **{'encoder.params': torch.zeros(1000)})
    with pytest.raises(FormatError, match=r'1000 .*1184'):
        m.load_state_dict(sd)


def test_unsupported_options_name_themselves():
    from videoswap_amd.atlas import HashGridMLP
    with pytest.raises(NotImplementedError, match='fp16'):
        HashGridMLP(2, 3, fp16=True)
    with pytest.raises(NotImplementedError, match='input_dim'):
        HashGridMLP(3, 3)
    with pytest.raises(NotImplementedError, match='tcnn'):
        HashGridMLP(2, 3, mlp_type='tcnn')
    with pytest.raises(NotImplementedError, match='n_features_per_level'):
        HashGridMLP(2, 3, grid=dict(SMALL_GRID, n_features_per_level=4))


TOY = dict(res_x=48, res_y=32, T=4)


@pytest.fixture(scope='module')
def toy():
    return arc.toy_models(arc.toy_config())


def test_render_matches_the_reference_loop_in_fp64(toy):
    """Bound: the renderer runs the networks in fp32, the yardstick in fp64.  An fp32 network of this depth carries about
    1e2 x 2^-24 ~ 1e-5 of error into (u, v); the toy texture (finest level 31 cells per unit, table within +-0.5, weights
    at twice the default scale) turns a (u, v) error into colour with a slope of the order of 1e2: 1e-3 on values in [0, 1].
    That slope is the texture's alone: uv_fg, uv_bg and alpha are plain fp32 network outputs and are held to 1e-5."""
    from videoswap_amd import atlas
    frames = [0, 1, 2, 3]
    with standin():
        got = atlas.render_atlas(toy, TOY['res_x'], TOY['res_y'], TOY['T'], frames=frames)
    want = arc.ref_render(toy, TOY['res_x'], TOY['res_y'], TOY['T'], frames, torch.float64)
    assert got['reconstruction'].shape == (4, 32, 48, 3) and got['alpha'].shape == (4, 32, 48)
    assert got['uv_fg'].shape == got['uv_bg'].shape == (4, 32, 48, 2)
    for k in ('reconstruction', 'alpha', 'uv_fg', 'uv_bg'):
        err = float((got[k].double() - want[k]).abs().max())
        print(f'render vs fp64 reference loop, {k}: {err:.3e}')
        assert err <= (1e-3 if k == 'reconstruction' else 1e-5), (k, err)
    assert float(want['reconstruction'].std()) > 0.02 and float(want['alpha'].std()) > 0.01      # not a constant image
    assert 0.001 <= float(got['alpha'].min()) and float(got['alpha'].max()) <= 0.991
    # a subset of frames is the same pixels
    with standin():
        sub = atlas.render_atlas(toy, TOY['res_x'], TOY['res_y'], TOY['T'], frames=[3, 1])
    assert torch.equal(sub['reconstruction'], got['reconstruction'][[3, 1]])


def test_four_launches_per_chunk_whatever_the_frame_count(toy):
    from videoswap_amd import atlas
    n = TOY['res_x'] * TOY['res_y']
    for frames, rows, chunks in (([0], 1 << 20, 1), ([0, 1, 2, 3], 1 << 20, 1), ([0, 1, 2, 3], 2 * n, 2), ([0, 1, 2], 1000, 5)):
        with standin() as (c, h):
            out = atlas.render_atlas(toy, TOY['res_x'], TOY['res_y'], TOY['T'], frames=frames, rows_per_call=rows)
        assert c.calls == 3 * chunks and h.calls == chunks and out['launches'] == 4 * chunks
        assert sum(h.rows) == 2 * len(frames) * n                               # FG and BG queries of a chunk in ONE launch


def test_psnr_of_a_constant_offset():
    from videoswap_amd.atlas import atlas_psnr
    frames = torch.rand(3, 8, 10, 3, dtype=torch.float64) * 0.8
    per_frame, mean = atlas_psnr(frames + 0.1, frames)
    assert per_frame.dtype == torch.float64 and per_frame.shape == (3,)
    assert float((per_frame - 20.0).abs().max()) <= 1e-9 and abs(mean - 20.0) <= 1e-9


def _area_direct(mapping, F_Alpha, mask_frames, resx, T, uv_shift, invert_alpha, alpha_thresh):
    """get_mapping_area restated directly: mask_frames [H, W, T] as the reference holds it, one batch"""
    relis_i, relis_j, relis_f = torch.where(mask_frames)
    relis = relis_i.unsqueeze(1) / (resx / 2) - 1
    reljs = relis_j.unsqueeze(1) / (resx / 2) - 1
    relfs = relis_f.unsqueeze(1) / (T / 2) - 1
    xyt = torch.cat((reljs, relis, relfs), dim=1)
    with torch.no_grad():
        uv, alpha = mapping(xyt), F_Alpha(xyt).squeeze()
    if invert_alpha:
        alpha = -alpha
    minx = miny = 1.0
    maxx = maxy = -1.0
    if bool(torch.any(alpha > alpha_thresh)):
        uv = uv * 0.5 + uv_shift
        sel = uv[alpha > alpha_thresh]
        minx, miny = min(minx, float(sel[:, 0].min())), min(miny, float(sel[:, 1].min()))
        maxx, maxy = max(maxx, float(sel[:, 0].max())), max(maxy, float(sel[:, 1].max()))
    maxx, maxy, minx, miny = min(maxx, 1), min(maxy, 1), max(minx, -1), max(miny, -1)
    return maxx, minx, maxy, miny, max(maxx - minx, maxy - miny)


def test_mapping_area_against_a_direct_restatement(toy):
    from videoswap_amd import atlas
    W, H, T = TOY['res_x'], TOY['res_y'], TOY['T']
    g = torch.Generator().manual_seed(5)
    masks = torch.rand(T, H, W, generator=g) > 0.6
    FG, BG, F_Alpha = toy['FG_UV_Mapping'], toy['BG_UV_Mapping'], toy['F_Alpha']
    with standin():
        a_all = float(F_Alpha(torch.rand(2000, 3, generator=g) * 2 - 1).median())
        cases = ((FG, 0.5, masks, False, a_all),                                # a threshold that splits the pixels
                 (BG, -0.5, None, True, -0.5),                                  # the background box of evaluate_model
                 (FG, 0.5, masks, False, 0.95),                                 # the foreground box of evaluate_model
                 (FG, 0.5, masks, False, 2.0))                                  # nothing passes: the (1, -1) start survives the clamp
        for mapping, shift, m, inv, thr in cases:
            got = atlas.mapping_area(mapping, F_Alpha, W, H, T, shift, masks=m, invert_alpha=inv, alpha_thresh=thr, rows_per_call=1500)
            ref_mask = (torch.ones(H, W, T) > 0) if m is None else m.permute(1, 2, 0)
            want = _area_direct(mapping, F_Alpha, ref_mask, max(W, H), T, shift, inv, thr)
            assert got == pytest.approx(want, abs=1e-6), (shift, inv, thr)
            assert all(-1 <= v <= 1 for v in got[:4])
    assert atlas.mapping_area.__doc__ and got[4] == -2.0


def test_mapping_area_takes_the_time_coordinate_as_the_reference_does(toy):
    """get_mapping_area:160 divides the integer frame tensor and subtracts 1 in fp32 (two roundings); evaluate_model
    rounds a Python float once.  T = 7: the two differ by an ulp at four of the seven frames."""
    from videoswap_amd import atlas
    W, H, T = 6, 4, 7
    seen = []

    class Recorder(torch.nn.Module):
        def __init__(self, inner):
            super().__init__()
            self.inner = inner

        def forward(self, xyt):
            seen.append(xyt.clone())
            return self.inner(xyt)

    want = torch.arange(T) / (T / 2) - 1
    once = torch.tensor([f / (T / 2) - 1 for f in range(T)], dtype=torch.float64).to(torch.float32)
    assert int((want != once).sum()) == 4                                      # the case can tell the two apart
    with standin():
        atlas.mapping_area(Recorder(toy['FG_UV_Mapping']), toy['F_Alpha'], W, H, T, 0.5)
    xyt = torch.cat(seen)
    assert xyt.shape == (T * H * W, 3) and torch.equal(xyt[:, 2].reshape(T, H * W), want.unsqueeze(1).expand(T, H * W))
    assert torch.equal(atlas._pixel_axes(W, H, T, 'cpu')[2], once)             # the renderer keeps evaluate_model's form


def test_texture_is_the_reference_row_loop(toy):
    from videoswap_amd import atlas
    F_Atlas = toy['F_Atlas']
    with standin() as (_, h):
        tex = atlas.atlas_texture(F_Atlas, 20, -0.7, 0.4, 0.1, 0.9)
        assert h.calls == 1 and tex.shape == (20, 20, 3)
        indsx, indsy = torch.linspace(-0.7, 0.4, 20), torch.linspace(0.1, 0.9, 20)
        want = torch.zeros(20, 20, 3)
        with torch.no_grad():
            for k, i in enumerate(indsy):                                       # get_high_res_texture:97-100
                want[k] = F_Atlas(torch.cat((indsx.unsqueeze(1), i * torch.ones_like(indsx.unsqueeze(1))), dim=1))
        want = 0.5 * (want + 1)
    assert float((tex - want).abs().max()) <= 1e-6


def test_command_end_to_end_on_a_synthetic_checkpoint(tmp_path):
    """YAML + checkpoint in the reference's on-disk format (F_Atlas with the reference's own grid: 5 487 024 table
    values) -> the listed files; the frames handed in are the rendering itself, 8-bit, so the PSNR is that of the
    quantisation (above 50 dB)"""
    from PIL import Image

    from videoswap_amd import atlas, render_atlas
    config = arc.toy_config()
    models = arc.toy_models(config, grid=None, seed=3, table_range=0.5)
    W, H, T = 40, 24, 3
    cfg_path, ckpt_path = str(tmp_path / 'atlas.yml'), str(tmp_path / 'models_40000.pth')
    with open(cfg_path, 'w') as f:
        yaml.safe_dump({'name': 'toy', 'datasets': {'res_x': W, 'res_y': H, 'max_frames': T, 'frame_path': str(tmp_path / 'none')},
                        'models': config}, f)
    torch.save(dict({k: m.state_dict() for k, m in models.items()}, optimizer={'state': {}}, iteration=40000), ckpt_path)
    with standin():
        loaded = atlas.load_atlas_models(cfg_path, ckpt_path, names=atlas.RENDER_MODEL_NAMES)
        assert sorted(loaded) == sorted(atlas.RENDER_MODEL_NAMES) and isinstance(loaded['F_Atlas'], atlas.HashGridMLP)
        first = atlas.render_atlas(loaded, W, H, T)
    os.makedirs(tmp_path / 'frames')
    os.makedirs(tmp_path / 'masks')
    for f in range(T):
        img = (first['reconstruction'][f].clamp(0, 1) * 255).round().to(torch.uint8).numpy()
        Image.fromarray(img).save(str(tmp_path / 'frames' / f'{f:05d}.png'))
        Image.fromarray(((first['alpha'][f] > first['alpha'].median()).to(torch.uint8) * 255).numpy()).save(str(tmp_path / 'masks' / f'{f:05d}.png'))
    save = str(tmp_path / 'out')
    args = render_atlas.parse_args(['--atlas_config_path', cfg_path, '--atlas_model_path', ckpt_path, '--save_dir', save,
                                    '--frame_dir', str(tmp_path / 'frames'), '--mask_dir', str(tmp_path / 'masks'),
                                    '--frames', '0,2', '--texture_resolution', '32'])
    assert args.frames == [0, 2]
    with standin():
        summary = render_atlas.run(args, device=torch.device('cpu'))
    assert sorted(os.listdir(save)) == ['alpha', 'reconstruction', 'summary.json', 'texture_orig1.png', 'texture_orig2.png']
    assert sorted(os.listdir(os.path.join(save, 'reconstruction'))) == ['00000.png', '00002.png'] == sorted(os.listdir(os.path.join(save, 'alpha')))
    assert Image.open(os.path.join(save, 'reconstruction', '00002.png')).size == (W, H)
    assert Image.open(os.path.join(save, 'texture_orig1.png')).size == (32, 32)
    back = np.asarray(Image.open(os.path.join(save, 'reconstruction', '00002.png')), dtype=np.float32) / 255
    assert float(np.abs(back - first['reconstruction'][2].numpy()).max()) <= 0.5 / 255 + 1e-6
    with open(os.path.join(save, 'summary.json')) as f:
        on_disk = json.load(f)
    assert on_disk == json.loads(json.dumps(summary))
    assert on_disk['render_launches'] == 4 and on_disk['number_of_frames'] == T and on_disk['frames'] == [0, 2]
    assert sorted(on_disk['psnr_per_frame']) == ['00000', '00002'] and on_disk['psnr_mean'] > 50
    assert on_disk['foreground_box_uses_masks'] and set(on_disk['background_box']) == {'maxx', 'minx', 'maxy', 'miny', 'edge_size'}
    # a checkpoint whose table has another length: the first outside evidence about the restated level table
    from videoswap_amd.formats import FormatError
    bad = torch.load(ckpt_path, weights_only=False)
    bad['F_Atlas']['encoder.params'] = torch.zeros(5487024 + 16)
    torch.save(bad, str(tmp_path / 'bad.pth'))
    with pytest.raises(FormatError, match=r'F_Atlas.*5487040.*5487024'):
        atlas.load_atlas_models(cfg_path, str(tmp_path / 'bad.pth'), names=atlas.RENDER_MODEL_NAMES)
    with pytest.raises(SystemExit):
        render_atlas.parse_args(['--atlas_config_path', cfg_path, '--atlas_model_path', ckpt_path, '--save_dir', save, '--frames', 'a,b'])
