"""Atlas point propagation (videoswap_amd/atlas.py, propagate_points.py) — host side, no GPU.

`ops.coord_mlp` is replaced by the stand-in of tests/atlas_case.py (fp32 PyTorch on the weights UNPACKED from the kernel's
buffer) for the duration of a test.  The reference is propagate_point_displacement.py / IMLP_Hash themselves: re-run from
the reference tree when it is readable, read from tests/golden/atlas_propagate.pt otherwise
(tests/golden/make_golden_atlas.py).  The comparison rule for tracks is atlas_case.compare_tracks.
"""
import os

import pytest
import torch
import yaml

import atlas_case
from atlas_case import build_models, compare_tracks, standin, write_case


@pytest.fixture(scope='module')
def fix():
    data, origin = atlas_case.load_fixture()
    print('atlas fixture from the', origin)
    return data


def test_recorded_fixture_is_what_the_generator_makes(fix):
    """the committed file and a fresh run of the reference agree (only meaningful where the reference tree is readable)"""
    rec = torch.load(atlas_case.FIXTURE, map_location='cpu', weights_only=True)
    assert torch.equal(rec['pred_tracks'], fix['pred_tracks'])
    assert float((rec['alpha'] - fix['alpha']).abs().max()) <= 1e-6
    vis = float((rec['alpha'] > 0.5).float().mean())
    assert 0.25 <= vis <= 0.75                                                 # both visibility branches, a quarter each at least
    assert os.path.getsize(atlas_case.FIXTURE) < 1 << 20


def test_coord_mlp_equals_imlp_hash(fix):
    from videoswap_amd.atlas import CoordMLP
    assert len(fix['variants']) == 8
    seen = set()
    for v in fix['variants']:
        kw = v['kwargs']
        m = CoordMLP(**kw)
        assert sorted(m.state_dict()) == sorted(v['state_dict'])               # hidden.<i>.weight / hidden.<i>.bias
        m.load_state_dict(v['state_dict'])
        with standin() as s, torch.no_grad():
            y = m(v['x'])
        assert s.calls == 1 and y.shape == v['y'].shape
        err = float((y - v['y']).abs().max())
        assert err <= 2e-6, (kw, err)
        seen.add((kw['pe_type'], bool(kw['skip_layers']), kw['use_tanh']))
    assert len(seen) == 8


def test_packed_weights_are_cached_until_a_parameter_changes():
    from videoswap_amd.atlas import CoordMLP
    m = CoordMLP(3, 2, hidden_dim=32, mlp_layers=3)
    a = m.packed()
    assert m.packed() is a
    with torch.no_grad():
        m.hidden[1].bias.add_(1.0)
    b = m.packed()
    assert b is not a and not torch.equal(a, b)
    m.load_state_dict({k: v + 1 for k, v in m.state_dict().items()})
    assert m.packed() is not b


def test_unsupported_options_name_themselves():
    from videoswap_amd.atlas import CoordMLP
    with pytest.raises(NotImplementedError, match='hash_encoding'):
        CoordMLP(2, 3, pe_type='hash_encoding')
    with pytest.raises(NotImplementedError, match='tcnn'):
        CoordMLP(3, 2, mlp_type='tcnn')
    from videoswap_amd import ops
    with standin(), pytest.raises(NotImplementedError, match='hash_encoding'):
        ops.coord_mlp(torch.zeros(1, 3), torch.zeros(4), 3, 2, 32, 2, pe_type='hash_encoding')
    with standin(), pytest.raises(NotImplementedError, match='tcnn'):
        ops.coord_mlp(torch.zeros(1, 3), torch.zeros(4), 3, 2, 32, 2, mlp_type='tcnn')


def _propagate(fix, tmp, keep=None):
    from videoswap_amd import atlas
    models = build_models(fix)
    os.makedirs(str(tmp), exist_ok=True)
    src, tap, tgt = write_case(str(tmp), fix, keep)
    ds = fix['config']['datasets']
    with standin() as s:
        out, details = atlas.propagate_point_sequence(src, tap, tgt, *models, larger_dim=max(ds['res_x'], ds['res_y']),
                                                      number_of_frames=fix['number_of_frames'], return_details=True)
    return out, details, s


def test_propagation_matches_the_reference(fix, tmp_path):
    out, details, s = _propagate(fix, tmp_path)
    figures = compare_tracks(fix, out, details)
    print('propagation vs reference:', figures)
    assert figures['compared'] == 6 * fix['number_of_frames'] * 2
    name2id = fix['tap']['point_name2id']
    for k in ('p6', 'p7'):                                                    # not named by the target file: tracks kept
        assert torch.equal(out['pred_tracks'][:, name2id[k]], fix['tap']['pred_tracks'][:, name2id[k]])
    assert 'ghost' in fix['target_points'] and 'ghost' not in fix['source_points']
    assert fix['tap']['pred_tracks'].shape[0] > fix['number_of_frames']      # a TAP longer than the atlas
    assert torch.equal(out['point_embedding'], fix['tap']['point_embedding'])
    assert out['point_name2id'] == name2id
    both = out['pred_tracks'][:fix['number_of_frames'], [name2id[k] for k in details['names']], 0]
    assert bool((both == -1).any()) and bool((both != -1).any())             # both visibility branches were taken
    assert s.calls == 3


def test_propagation_of_a_single_point(fix, tmp_path):
    out, details, s = _propagate(fix, tmp_path, keep=['p3'])
    figures = compare_tracks(fix, out, details, names=['p3'])
    assert figures['compared'] == fix['number_of_frames'] * 2
    name2id = fix['tap']['point_name2id']
    for k in fix['source_points']:
        if k != 'p3':
            assert torch.equal(out['pred_tracks'][:, name2id[k]], fix['tap']['pred_tracks'][:, name2id[k]])


def test_kernel_calls_do_not_depend_on_the_number_of_points(fix, tmp_path):
    one = _propagate(fix, tmp_path / 'a', keep=['p0'])[2]
    case = dict(fix)
    case['target_points'] = {k: [v[0] + 7.0, v[1] - 5.0] for k, v in fix['source_points'].items()}     # all 8 dragged
    eight = _propagate(case, tmp_path / 'b')[2]
    T = fix['number_of_frames']
    assert one.calls == eight.calls == 3
    assert one.rows == [3, 3 * T, T] and eight.rows == [3 * 8, 3 * 8 * T, 8 * T]


def test_nothing_dragged_leaves_the_tap_alone(fix, tmp_path):
    out, details, s = _propagate(fix, tmp_path, keep=['ghost'])
    assert s.calls == 0 and details['names'] == []
    assert torch.equal(out['pred_tracks'], fix['tap']['pred_tracks'])


def test_cli_round_trip(fix, tmp_path):
    """config YAML + checkpoint (with entries propagation must ignore) -> TAP_<target stem>.pth, read back by load_tap"""
    from videoswap_amd import formats, propagate_points
    src, tap, tgt = write_case(str(tmp_path), fix)
    config = {'name': 'toy_atlas', 'mixed_precision': 'no',
              'datasets': dict(fix['config']['datasets'], frame_path=str(tmp_path / 'frames')),
              'models': dict(fix['config']['models'],
                             BG_UV_Mapping=dict(input_dim=3, output_dim=2, hidden_dim=64, pe_type='none', pe_dim=2,
                                                mlp_type='origin', mlp_layers=4, skip_layers=[]),
                             F_Atlas=dict(input_dim=2, output_dim=3, hidden_dim=64, pe_type='hash_encoding', pe_dim=10,
                                          mlp_type='origin', mlp_layers=8, skip_layers=[4, 7], fp16=False))}
    cfg_path, ckpt_path = str(tmp_path / 'atlas.yml'), str(tmp_path / 'models_40000.pth')
    with open(cfg_path, 'w') as f:
        yaml.safe_dump(config, f)
    torch.save(dict(fix['state_dicts'], BG_UV_Mapping={'hidden.0.weight': torch.zeros(64, 3)},
                    F_Atlas={'encoder.params': torch.zeros(100), 'hidden.0.weight': torch.zeros(64, 32)},
                    optimizer={'state': {}, 'param_groups': [{'lr': 1e-4}]}, iteration=40000), ckpt_path)
    # more frame files than max_frames: number_of_frames = min(max_frames, files)
    os.makedirs(tmp_path / 'frames')
    for i in range(fix['number_of_frames'] + 3):
        (tmp_path / 'frames' / f'{i:05d}.jpg').write_bytes(b'')
    argv = ['--atlas_config_path', cfg_path, '--atlas_model_path', ckpt_path, '--source_point_path', src,
            '--source_tap_path', tap, '--target_point_path', tgt]
    args = propagate_points.parse_args(argv)
    assert args.save_path == os.path.join(str(tmp_path), 'TAP_edit.pth')
    with standin():
        propagate_points.run(args, device=torch.device('cpu'))
    got = formats.load_tap(args.save_path)
    compare_tracks(fix, got, _propagate(fix, tmp_path / 'again')[1])          # the rule of the direct call
    assert torch.equal(got['point_embedding'], fix['tap']['point_embedding'])
    assert got['point_name2id'] == fix['tap']['point_name2id']
    # --num_frames stands in for the file count; --save_path overrides the default name
    other = str(tmp_path / 'elsewhere' / 'x.pth')
    args = propagate_points.parse_args(argv + ['--num_frames', '10', '--save_path', other])
    with standin():
        propagate_points.run(args, device=torch.device('cpu'))
    short = formats.load_tap(other)
    cols = [fix['tap']['point_name2id'][k] for k in fix['source_points'] if k in fix['target_points']]
    assert bool((short['pred_tracks'][10:, cols] == -1).all())
    with pytest.raises(SystemExit):
        propagate_points.parse_args([a if a != src else str(tmp_path / 'keyframe.json') for a in argv])


def test_config_with_an_unsupported_propagation_network_is_refused(fix, tmp_path):
    from videoswap_amd import atlas
    cfg = {'models': dict(fix['config']['models'])}
    cfg['models']['F_Alpha'] = dict(cfg['models']['F_Alpha'], mlp_type='tcnn')
    ckpt = str(tmp_path / 'm.pth')
    torch.save(fix['state_dicts'], ckpt)
    with pytest.raises(NotImplementedError, match='F_Alpha.*tcnn'):
        atlas.load_atlas_models(cfg, ckpt)


def test_point_files_are_y_x(fix, tmp_path):
    """swapping the two numbers of every point changes the result: the JSON order [y, x] is honoured"""
    out, details, _ = _propagate(fix, tmp_path / 'a')
    flipped = dict(fix)
    flipped['source_points'] = {k: [v[1], v[0]] for k, v in fix['source_points'].items()}
    flipped['target_points'] = {k: [v[1], v[0]] for k, v in fix['target_points'].items()}
    out2, details2, _ = _propagate(flipped, tmp_path / 'b')
    assert float((details['pixels'] - details2['pixels']).abs().max()) > 1.0
