"""Fitting atlas mapping networks, on the CPU: the host code of videoswap_amd/atlas_fit.py and the command
`python -m videoswap_amd.fit_inverse` on pure-PyTorch stand-ins of the two training ops (atlas_fit_case.FitStandin), the
pretrain_mapping fixture rule, and the proof that the gradient parity rule of tests/test_atlas_fit_gpu.py has power: it
rejects three planted wrong gradients, and the input selection keeps its cap on every GPU case's inputs."""
import copy
import os

import pytest
import torch
import yaml

import atlas_fit_case as case
from atlas_case import standin
from atlas_fit_case import fit_standin


def test_chunk_rows_and_workspace_come_from_the_library():
    from videoswap_amd import _lib, ops
    assert ops.COORD_MLP_WGRAD_ROWS == case.R == _lib.load().vsx_coord_mlp_wgrad_rows()
    saved, scratch, grad = ops.coord_mlp_train_workspace(1000, 3, 2, 256, 6)
    P = 3 * 256 + 256 + 4 * (256 * 256 + 256) + 2 * 256 + 2
    assert (saved, scratch, grad) == (1000 * (5 * 256 + 3 + 2), 2 * P + 2 * 1000 * 256 + 1000 * 2, P)
    with pytest.raises(NotImplementedError, match='tcnn'):
        ops.coord_mlp_train_workspace(10, 3, 2, 256, 6, mlp_type='tcnn')


def test_gradient_path_only_when_asked():
    m = case.network(dict(case.FG, hidden_dim=32, mlp_layers=3), 1.0, seed=1)
    x = torch.rand(9, 3) * 2 - 1
    with fit_standin() as s, standin() as plain:
        y = m(x)                                                    # training mode, parameters require grad, grad mode on
        assert y.grad_fn is None and plain.calls == 1 and s.forward_calls == 0
        assert m.differentiable_(True) is m
        y2 = m(x)
        assert y2.grad_fn is not None and s.forward_calls == 1 and plain.calls == 1 and torch.equal(y2.detach(), y)
        with torch.no_grad():
            assert m(x).grad_fn is None
        for q in m.parameters():
            q.requires_grad_(False)
        assert m(x).grad_fn is None
        assert s.forward_calls == 1 and plain.calls == 3
        for q in m.parameters():
            q.requires_grad_(True)
        with pytest.raises(NotImplementedError, match='input gradients'):
            m(x.clone().requires_grad_(True))
        assert m.differentiable_(False) is m and m(x).grad_fn is None


@pytest.mark.parametrize('kw', [dict(case.FG, hidden_dim=64), dict(case.SKIP, hidden_dim=32), dict(case.ALPHA, hidden_dim=32, mlp_layers=3),
                                dict(case.INV, use_tanh=False, hidden_dim=32, mlp_layers=2)], ids=['fg', 'skip', 'alpha', 'no_tanh'])
def test_autograd_function_on_the_standin_matches_autograd(kw):
    """the layout of `grad` (unpadded, nn.Linear order), the views handed to the parameters, repacking after a step"""
    m = case.network(kw, 1.5, seed=3).differentiable_(True)
    x, dropped, _ = case.select_inputs(m, 200, seed=4)
    G = case.cotangent(200, kw['output_dim'], seed=4)
    g64, g32 = case.reference_grads(m, x, G, torch.float64), case.reference_grads(m, x, G, torch.float32)
    with fit_standin() as s:
        y, grads = case.backward_through(m, x, G)
        assert (s.forward_calls, s.backward_calls) == (1, 1)
        for q, g in zip(m.parameters(), grads):
            assert g.shape == q.shape
        e_torch, e_standin = case.worst_error(g32, g64), case.worst_error(grads, g64)
        assert e_standin <= 4 * e_torch, (e_standin, e_torch)
        before = m.packed().clone()
        torch.optim.SGD(m.parameters(), lr=0.1).step()
        assert not torch.equal(m.packed(), before)                  # the `_version` key saw the step


@pytest.mark.parametrize('plant', ['drop_row', 'wrong_mask', 'no_tanh'])
def test_the_rule_rejects_a_planted_wrong_gradient(plant):
    kw = dict(case.FG, hidden_dim=64, mlp_layers=4)
    m = case.network(kw, 2.0, seed=8).differentiable_(True)
    x, _, _ = case.select_inputs(m, 1000, seed=9)
    G = case.cotangent(1000, 2, seed=9)
    g64, g32 = case.reference_grads(m, x, G, torch.float64), case.reference_grads(m, x, G, torch.float32)
    e_torch = case.worst_error(g32, g64)
    with fit_standin() as good:
        _, grads = case.backward_through(m, x, G)
    assert good.backward_calls == 1 and case.worst_error(grads, g64) <= 4 * e_torch
    with fit_standin(plant):
        _, wrong = case.backward_through(m, x, G)
    e_wrong = case.worst_error(wrong, g64)
    print(f'{plant}: E {e_wrong:.3e} against the bound {4 * e_torch:.3e}')
    assert e_wrong > 4 * e_torch


def test_input_selection_keeps_its_cap_on_every_gpu_case():
    shares = {}
    for (name, kw, N, scale), rid in zip(case.RUNS, case.RUN_IDS):
        m = case.network(kw, scale, seed=N % 1000 + len(name))
        x, dropped, delta = case.select_inputs(m, N, seed=N)        # asserts the cap
        assert x.shape == (N, kw['input_dim']) and 0 < delta < 1e-3
        shares[rid] = round(dropped, 3)
    print('dropped shares:', shares)


def test_pretrain_mapping_follows_the_reference_on_the_standin():
    with fit_standin() as s:
        case.check_pretrain_fixture('cpu')
    assert s.backward_calls == 3 * 3 * 2                            # seeds x iterations x frames: one backward call per step


def test_inverse_fit_on_the_standin():
    nets = case.fit_networks()
    with fit_standin() as s:
        res = case.run_fit(nets, 'cpu')
    hist = res['loss_history']
    assert len(hist) == case.FIT['iters'] and res['steps_skipped'] == 0 and s.backward_calls == case.FIT['iters']
    assert hist[-1] < hist[0]
    assert 0 < res['holdout_rows'] < 512 and res['roundtrip_max_px'] >= res['roundtrip_mean_px'] > 0
    h64 = case.fit_fp64(nets)
    print('inverse fit: first / last loss', hist[0], hist[-1], 'fp32 stand-in vs fp64 restatement', case.history_diff(hist, h64))
    assert case.history_diff(hist, h64) < 1e-4                      # the same steps: six digits of a loss of O(1)
    with fit_standin() as s:                                        # F_Alpha says background everywhere: every step is skipped
        res = case.run_fit(case.fit_networks(alpha_shift=-50.0), 'cpu', iters=3)
    assert res['loss_history'] == [] and res['steps_skipped'] == 3 and s.backward_calls == 0
    assert res['holdout_rows'] == 0 and res['roundtrip_mean_px'] != res['roundtrip_mean_px']


def _write_atlas(tmp, with_inverse_spec, with_inverse_weights):
    """an atlas as the commands read it: YAML + checkpoint (the fixture of the propagation tests, its inverse removed)"""
    import atlas_case
    fix = torch.load(atlas_case.FIXTURE, map_location='cpu', weights_only=True)
    config = copy.deepcopy(fix['config'])
    if not with_inverse_spec:
        del config['models']['FG_UV_Mapping_Inverse']
    ckpt = {k: v for k, v in fix['state_dicts'].items() if with_inverse_weights or k != 'FG_UV_Mapping_Inverse'}
    ckpt['F_Atlas'] = {'encoder.params': torch.arange(6.0)}           # entries the tool does not touch
    ckpt['note'] = 'kept'
    cfg_path, ckpt_path = os.path.join(tmp, 'atlas.yml'), os.path.join(tmp, 'models.pth')
    with open(cfg_path, 'w') as f:
        yaml.safe_dump(config, f)
    torch.save(ckpt, ckpt_path)
    return fix, cfg_path, ckpt_path


@pytest.mark.parametrize('with_spec', [True, False], ids=['yaml_has_inverse', 'yaml_without_inverse'])
def test_cli_end_to_end(tmp_path, with_spec):
    import atlas_case
    from videoswap_amd import atlas, fit_inverse, formats
    fix, cfg_path, ckpt_path = _write_atlas(str(tmp_path), with_spec, with_inverse_weights=with_spec)
    save = str(tmp_path / 'out' / 'models_inv.pth')
    args = fit_inverse.build_parser().parse_args(['--atlas_config_path', cfg_path, '--atlas_model_path', ckpt_path, '--save_path', save,
                                                  '--iters', '4', '--batch', '512', '--seed', '3', '--num_frames', str(fix['number_of_frames'])])
    with fit_standin() as s:
        res = fit_inverse.run(args, device='cpu')
        assert s.backward_calls == len(res['loss_history']) == 4
        out = formats._load(save)
        before = formats._load(ckpt_path)
        assert set(out) == set(before) | {'FG_UV_Mapping_Inverse'} and out['note'] == 'kept'
        for k in ('FG_UV_Mapping', 'F_Alpha', 'F_Atlas'):
            assert all(torch.equal(out[k][n], before[k][n]) for n in before[k])
        assert sorted(out['FG_UV_Mapping_Inverse']) == sorted(fix['state_dicts']['FG_UV_Mapping_Inverse'])
        if with_spec:                                                # it started from the checkpoint's inverse and moved it
            assert not torch.equal(out['FG_UV_Mapping_Inverse']['hidden.0.weight'], before['FG_UV_Mapping_Inverse']['hidden.0.weight'])
        assert res['config_path'] == str(tmp_path / 'out' / 'models_inv.yml')
        used = atlas.load_atlas_config(res['config_path'])
        assert used['models']['FG_UV_Mapping_Inverse'] == dict(fix['config']['models']['FG_UV_Mapping'], output_dim=3)
        # propagate_points' own loading and propagation accept the pair
        models = atlas.load_atlas_models(res['config_path'], save, device='cpu')
        src, tap, tgt = atlas_case.write_case(str(tmp_path), fix)
        ds = fix['config']['datasets']
        got = atlas.propagate_point_sequence(src, tap, tgt, *(models[k] for k in atlas.MODEL_NAMES),
                                             larger_dim=max(ds['res_x'], ds['res_y']), number_of_frames=fix['number_of_frames'])
    assert got['pred_tracks'].shape == fix['pred_tracks'].shape


def test_cli_reads_masks_as_the_reference_does(tmp_path):
    from PIL import Image
    from videoswap_amd import atlas
    import numpy as np
    for i in range(3):
        a = np.zeros((6, 8), dtype=np.uint8)
        a[:, :4 + i] = 255
        a[0, 0] = 254                                                # not exactly 1 after / 255: background
        Image.fromarray(a).save(str(tmp_path / f'{i:05d}.png'))
    masks = atlas.load_mask_frames(str(tmp_path), 8, 6, 2)
    assert masks.shape == (6, 8, 2) and masks.dtype == torch.float32
    assert int((masks[:, :, 0] == 1).sum()) == 6 * 4 - 1 and int((masks[:, :, 1] == 1).sum()) == 6 * 5 - 1
    with pytest.raises(FileNotFoundError):
        atlas.load_mask_frames(str(tmp_path), 8, 6, 4)
