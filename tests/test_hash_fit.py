"""The gradient path of HashGridMLP on the CPU, through stand-ins of the four new ops (hash_fit_case.HashFitStandin): the
autograd wiring, the switch, which gradients are asked for, atlas.fit_reconstruction, the power of the comparison rule
against planted errors, and the refit_atlas command on a toy atlas.  The kernels themselves: tests/test_hash_fit_gpu.py and
tests/test_hash_fit_cpu_check.py."""
import os

import pytest
import torch
import yaml

import atlas_render_case as arc
import hash_fit_case as hc


def _case(stack='h64', grid='small-half', N=65, scale=1.0, seed=5, one_cell=False):
    cfg, family = hc.GRIDS[grid]
    m = hc.network(hc.STACKS[stack], cfg, family, scale, seed)
    x, dropped, _ = hc.select_inputs(m, N, seed, one_cell=one_cell)
    G = hc.cotangent(N, m.output_dim, seed)
    return m, x, G, dropped


def test_the_four_ops_are_published_and_swappable():
    from videoswap_amd import ops
    for name in ('hash_grid_backward', 'hash_mlp_train_workspace', 'hash_mlp_train_forward', 'hash_mlp_backward'):
        assert name in ops._raw and callable(getattr(ops, name))
    assert hc.HashFitStandin.hash_mlp_train_workspace(0, arc.SMALL_GRID, 3, 64, 4, [2]) == (0, 0, 64 * 8 + 64 + 64 * 64 + 64 + 64 * 72 + 64 + 3 * 64 + 3)


def test_the_restatement_is_the_forward_restatement_left_attached():
    m, x, _, _ = _case()
    for dtype in (torch.float32, torch.float64):
        want = arc.hash_encode(x, m.encoder.params, m.grid, dtype)
        got = hc.hash_encode_diff(x.to(dtype), m.encoder.params.detach().to(dtype), m.grid, dtype)
        assert torch.equal(got, want)


@pytest.mark.parametrize('stack,grid', [('h64', 'small-half'), ('h32', 'g16-scaled'), ('no_tanh', 'g20-scaled')])
def test_autograd_wiring_gives_the_reference_gradients(stack, grid):
    m, x, G, _ = _case(stack, grid)
    g64 = hc.reference_grads(m, x, G, torch.float64)
    e32 = hc.worst_error(hc.reference_grads(m, x, G, torch.float32), g64)
    with hc.hash_fit_standin() as s:
        m.differentiable_(True)
        y, grads = hc.backward_through(m, x, G)
        assert s.forward_calls == 1 and s.backward_calls == 1 and s.wanted == [(True, True)]
        with torch.no_grad():
            assert torch.equal(y, m(x))                   # the training forward's output is the plain forward's
    e = hc.worst_error(grads, g64)
    print(f'{stack} {grid}: E_standin {e:.3g}  E_fp32torch {e32:.3g}')
    assert e <= 4 * e32


def test_flag_off_is_the_plain_call_and_the_switch_needs_grad_mode():
    m, x, _, _ = _case()
    with hc.hash_fit_standin() as s:
        y = m(x.clone().requires_grad_(True))             # off by default
        assert y.grad_fn is None and s.forward_calls == 0
        m.differentiable_(True)
        with torch.no_grad():
            assert m(x).grad_fn is None and s.forward_calls == 0
        m.requires_grad_(False)
        assert m(x).grad_fn is None and s.forward_calls == 0     # nothing requires grad
        assert m(x.clone().requires_grad_(True)).grad_fn is not None and s.forward_calls == 1
        assert m.differentiable_(False) is m and m(x.clone().requires_grad_(True)).grad_fn is None


def test_frozen_table_and_frozen_input_each_skip_their_gradient():
    m, x, G, _ = _case()
    m.differentiable_(True)
    with hc.hash_fit_standin() as s:
        m.encoder.params.requires_grad_(False)
        xg = x.clone().requires_grad_(True)
        (m(xg) * G).sum().backward()
        assert s.wanted[-1] == (False, True) and m.encoder.params.grad is None and xg.grad is not None
        m.encoder.params.requires_grad_(True)
        m.zero_grad()
        (m(x) * G).sum().backward()
        assert s.wanted[-1] == (True, False) and m.encoder.params.grad is not None
        m.requires_grad_(False)
        m.hidden[0].weight.requires_grad_(True)
        (m(x) * G).sum().backward()
        assert s.wanted[-1] == (False, False)


@pytest.mark.parametrize('plant', hc.PLANTS)
def test_the_rule_catches_planted_errors(plant):
    """each planted error must break E <= 4 E_fp32torch; 'skip_passes' needs a skip layer (h64: layer 2)"""
    m, x, G, _ = _case('h64', 'small-half', N=65)
    g64 = hc.reference_grads(m, x, G, torch.float64)
    e32 = hc.worst_error(hc.reference_grads(m, x, G, torch.float32), g64)
    m.differentiable_(True)
    with hc.hash_fit_standin(plant):
        _, grads = hc.backward_through(m, x, G)
    e = hc.worst_error(grads, g64)
    print(f'{plant}: E {e:.3g} against 4 x {e32:.3g}')
    assert e > 4 * e32


def test_grid_backward_stand_in_alone_matches_autograd():
    m, x, _, _ = _case('h32', 'g16-scaled', N=63)
    ge = torch.randn(63, 32, generator=torch.Generator().manual_seed(1))
    xd, td = x.double().requires_grad_(True), m.encoder.params.detach().double().requires_grad_(True)
    want_t, want_x = torch.autograd.grad((hc.hash_encode_diff(xd, td, m.grid, torch.float64) * ge.double()).sum(), [td, xd])
    gt, gx = hc.HashFitStandin().hash_grid_backward(x, ge, m.encoder.params.detach(), m.grid)
    # the fp32 position scale x + 0.5 is rounded at 2^-24 of scale_max = 2005 (each of the two weights of a corner carries
    # that absolute error) and a row's sum has 64 terms: 8 scale_max 2^-24 = 1e-3 of the largest element; a wrong corner is O(1)
    bound = 8 * hc.levels(m.grid)[-1]['scale'] * 2.0 ** -24
    assert float((gt.double() - want_t).abs().max()) <= bound * float(want_t.abs().max())
    assert float((gx.double() - want_x).abs().max()) <= bound * float(want_x.abs().max())
    assert bool((gt[~hc.addressed(m, x)] == 0).all())


def test_reconstruction_losses_evaluate_the_texture_once_and_restate_the_reference():
    from videoswap_amd import atlas
    models, video, masks = hc.toy_atlas()
    xyt = torch.rand(200, 3, generator=torch.Generator().manual_seed(2)) * 2 - 1
    rgb, agt = torch.rand(200, 3, generator=torch.Generator().manual_seed(3)), (torch.rand(200, 1, generator=torch.Generator().manual_seed(4)) > 0.5).float()
    with arc.standin() as (_, h), torch.no_grad():
        total, d = atlas.reconstruction_losses(models, xyt, rgb, agt, None, with_alpha_loss=True)
        assert h.calls == 1 and h.rows == [400]
        total2, d2 = atlas.reconstruction_losses(models, xyt, rgb, agt, None, with_alpha_loss=False)
        uv1, uv2 = models['FG_UV_Mapping'](xyt), models['BG_UV_Mapping'](xyt)
        a = 0.5 * (models['F_Alpha'](xyt) + 1.0) * 0.99 + 0.001
        fg, bg = (models['F_Atlas'](uv1 * 0.5 + 0.5) + 1) * 0.5, (models['F_Atlas'](uv2 * 0.5 - 0.5) + 1) * 0.5
    rgb_loss = (torch.norm(fg * a + bg * (1 - a) - rgb, dim=1) ** 2).mean()
    alpha_loss = torch.mean(-agt * torch.log(a) - (1 - agt) * torch.log(1 - a))
    sparsity = (torch.norm(fg * (1 - a), dim=1) ** 2).mean()
    assert sorted(d) == ['alpha_loss', 'rgb_loss', 'sparsity_loss', 'total_loss'] and 'alpha_loss' not in d2
    assert float(total) == pytest.approx(float(5000 * rgb_loss + 2000 * alpha_loss + 1000 * sparsity), rel=1e-5)
    assert float(total2) == pytest.approx(float(5000 * rgb_loss + 1000 * sparsity), rel=1e-5)


def test_fit_reconstruction_lowers_its_loss_and_leaves_the_other_networks_alone():
    models, video, masks = hc.toy_atlas()
    before = {k: {n: v.clone() for n, v in m.state_dict().items()} for k, m in models.items()}
    with hc.hash_fit_standin() as s:
        history, nets = hc.run_fit(models, video, masks, 'cpu', train=('F_Atlas',), iters=12, batch=512, lr=1e-3)
        assert s.forward_calls == 12 and s.backward_calls == 12 and set(s.wanted) == {(True, False)}   # frozen mappings: no grad_x
    assert len(history) == 12 and history[-1] < history[0]
    for k, m in nets.items():
        same = all(torch.equal(v, before[k][n]) for n, v in m.state_dict().items())
        assert same == (k != 'F_Atlas'), k
        assert all(q.requires_grad for q in m.parameters()) and not m._differentiable      # settings are back
    with hc.hash_fit_standin() as s:
        history, nets = hc.run_fit(models, video, masks, 'cpu', iters=6, batch=512, lr=1e-3)
        assert set(s.wanted) == {(True, True)}                                             # grad_x drives the mappings
    assert history[-1] < history[0]
    for k in hc.FIT_NETWORKS:
        assert not all(torch.equal(v, before[k][n]) for n, v in nets[k].state_dict().items()), k
    assert all(torch.equal(v, before['FG_UV_Mapping_Inverse'][n]) for n, v in nets['FG_UV_Mapping_Inverse'].state_dict().items())
    from videoswap_amd import atlas
    with pytest.raises(ValueError, match='FG_UV_Mapping_Inverse'):
        atlas.fit_reconstruction(models, video, masks, 1, train=('FG_UV_Mapping_Inverse',))


def test_fit_reconstruction_follows_its_fp64_restatement():
    models, video, masks = hc.toy_atlas()
    h64 = hc.fit_fp64(models, video, masks)
    with hc.hash_fit_standin():
        h32, _ = hc.run_fit(models, video, masks, 'cpu')
    diff = hc.history_diff(h32, h64)
    print(f'fit_reconstruction, fp32 stand-ins vs fp64: {diff:.3g} on losses of {h64[0]:.6g} .. {h64[-1]:.6g}')
    # before any update the two differ by fp32 rounding alone: the loss is a mean over 1024 rows of O(1) terms, 16 ulp of it.
    # From then on Adam's normalised step (lr g / (|g| + eps): a parameter whose gradient is rounding noise still moves by lr)
    # and ReLU masks that flip carry the rounding forward; the history stays within 1e-3 of the loss, where a wrong gradient
    # (the planted errors above are O(1) of a tensor) moves it by percents within a few steps.  The GPU test compares the
    # kernels' run with THIS run's distance instead of a constant.
    assert abs(h32[0] - h64[0]) <= 16 * 2.0 ** -24 * h64[0]
    assert h64[-1] < h64[0] and h32[-1] < h32[0] and diff <= 1e-3 * h64[0]


def test_refit_command_round_trip_on_a_toy_atlas(tmp_path):
    from PIL import Image

    from videoswap_amd import atlas, refit_atlas
    config = arc.toy_config()
    models = arc.toy_models(config, grid=None, seed=3, table_range=0.5)
    W, H, T = 40, 24, 3
    cfg_path, ckpt_path, out_path = str(tmp_path / 'atlas.yml'), str(tmp_path / 'models_40000.pth'), str(tmp_path / 'out' / 'refit.pth')
    with open(cfg_path, 'w') as f:
        yaml.safe_dump({'name': 'toy', 'datasets': {'res_x': W, 'res_y': H, 'max_frames': T, 'frame_path': str(tmp_path / 'none')},
                        'models': config}, f)
    torch.save(dict({k: m.state_dict() for k, m in models.items()}, optimizer={'state': {}}, iteration=40000), ckpt_path)
    os.makedirs(tmp_path / 'frames')
    os.makedirs(tmp_path / 'masks')
    g = torch.Generator().manual_seed(9)
    for f in range(T):
        Image.fromarray((torch.rand(H, W, 3, generator=g) * 255).to(torch.uint8).numpy()).save(str(tmp_path / 'frames' / f'{f:05d}.png'))
        Image.fromarray(((torch.rand(H, W, generator=g) > 0.5).to(torch.uint8) * 255).numpy()).save(str(tmp_path / 'masks' / f'{f:05d}.png'))
    args = refit_atlas.parse_args(['--atlas_config_path', cfg_path, '--atlas_model_path', ckpt_path, '--frame_dir', str(tmp_path / 'frames'),
                                   '--mask_dir', str(tmp_path / 'masks'), '--iters', '3', '--save_path', out_path, '--batch', '256',
                                   '--lr', '1e-3', '--seed', '4'])
    assert args.train == ('F_Atlas',)
    with hc.hash_fit_standin():
        history = refit_atlas.run(args, device=torch.device('cpu'))
        assert len(history) == 3
        ckpt = torch.load(out_path, weights_only=False)
        assert ckpt['iteration'] == 40000 and sorted(ckpt) == sorted(list(models) + ['optimizer', 'iteration'])
        for k, m in models.items():                       # only F_Atlas moved; the other tools load the file
            same = all(torch.equal(v, ckpt[k][n]) for n, v in m.state_dict().items())
            assert same == (k != 'F_Atlas'), k
        loaded = atlas.load_atlas_models(cfg_path, out_path, names=atlas.RENDER_MODEL_NAMES)
        assert atlas.render_atlas(loaded, W, H, T, frames=[1])['reconstruction'].shape == (1, H, W, 3)
    with pytest.raises(SystemExit):
        refit_atlas.run(refit_atlas.parse_args(['--atlas_config_path', cfg_path, '--atlas_model_path', ckpt_path, '--frame_dir', 'x',
                                                '--mask_dir', 'y', '--iters', '1', '--save_path', out_path, '--train', 'F_Atlas,Nope']))
