"""The full atlas training step on the CPU: the restatement of atlas_train_case.py pinned to the reference's own loss code
(tests/golden/atlas_train_losses.pt), and the host side (atlas_fit.AtlasLossFunction, training_losses, fit_atlas) through
CPU stand-ins of the two new ops: the row layout, which network sees which block, the loss_dict keys, the convention for a
flow term without a relevant row, the refusals, and the power of the parity rule against planted errors.  The kernels
themselves: tests/test_atlas_train_gpu.py and tests/test_atlas_train_cpu_check.py."""
import copy
import os

import pytest
import torch

import atlas_train_case as tc
from atlas_case import counted
from util import load_golden

NETS = tc.STEP_NETWORKS


def test_the_two_ops_are_published_and_swappable():
    from videoswap_amd import _lib, ops
    for name in ('atlas_batch', 'atlas_losses'):
        assert name in ops._raw and callable(getattr(ops, name))
    assert ops.ATLAS_LOSSES == tc.LOSSES and _lib.VSX_ABI_VERSION == 17
    assert ctypes_size(_lib.AtlasLossCfg) == 15 * 8


def ctypes_size(struct):
    import ctypes
    return ctypes.sizeof(struct)


def _golden():
    """(the recorded fixture, the same fixture re-run through the reference's loss code on THIS machine from the recorded
    inputs, or None where the reference's tree is not readable).  fp32 bits are a property of the machine as well as of the
    arithmetic (vector width decides the order of a reduction and the form of sin / tanh / log), so bit-equality in fp32 can
    only be asked against a run of the reference on the machine the test runs on."""
    import importlib.util
    from util import GOLDEN
    fix = load_golden('atlas_train_losses.pt')
    spec = importlib.util.spec_from_file_location('make_golden_atlas_train', os.path.join(GOLDEN, 'make_golden_atlas_train.py'))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return fix, (gen.generate(fix['data'], fix['idx']) if gen.reference_available() else None)


def _restated(fix, flags, dtype):
    c = fix['case']
    ev = tc.NetEval(tc.TinyNets(dtype), dtype)
    q = tc.Queries.from_data(tc.jif_of(fix['idx'], c['H'], c['W']), fix['data'], c['derivative_amount'], c['global_derivative_amount'])
    total, loss_dict = tc.step_restated(ev, q, fix['train'], *flags, dtype)
    total.backward()
    return ev, loss_dict


def _close(a, b, rel):
    return float((a.detach().double() - b.double()).abs().max()) <= rel * float(b.double().abs().max())


@pytest.mark.parametrize('flags', [(True, True), (False, False)], ids=['alpha+global', 'neither'])
def test_the_restatement_is_the_references_loss_code(flags):
    """every loss and every gradient with respect to a network output: 1e-12 relative in fp64 against the recorded run and
    against a re-run of the reference here; bit for bit in fp32 against the re-run here (the reference's tree is readable
    wherever the CPU suite is judged); against the recorded fp32 run, which another machine made with another vector width,
    the fp32 restatement must be as close to the recorded fp64 run as 4 x the recorded fp32 run is (floor: 2^-24)."""
    fix, here = _golden()
    c = fix['case']
    assert c == tc.GOLDEN_CASE and fix['data']['video_frames'].shape == (c['H'], c['W'], 3, c['T'])
    for tag, dtype in (('fp64', torch.float64), ('fp32', torch.float32)):
        ev, loss_dict = _restated(fix, flags, dtype)
        for name, order in tc.CALL_ORDER.items():
            order = [b for b in order if flags[1] or b != (5, 6)]
            assert [tag_ for n, tag_, _ in ev.calls if n == name] == order        # the reference's calls, in its order
        for source, want in (('recorded', fix['runs'][(flags, tag)]), ('here', here['runs'][(flags, tag)] if here else None)):
            if want is None:
                continue
            assert set(loss_dict) == set(want['loss_dict'])
            same_machine = source == 'here'
            want64 = fix['runs'][(flags, 'fp64')]
            for name in tc.CALL_ORDER:
                got = ev.outputs(name)
                assert len(got) == len(want['grads'][name])
                for k, (y, g_ref) in enumerate(zip(got, want['grads'][name])):
                    if dtype == torch.float64:
                        assert _close(y.grad, g_ref, 1e-12), (source, name, k)
                    elif same_machine:
                        assert torch.equal(y.grad, g_ref), (source, name, k)      # bit for bit
                    else:
                        g64 = want64['grads'][name][k]
                        top = float(g64.abs().max())
                        assert float((y.grad.double() - g64).abs().max()) <= 4 * max(float((g_ref.double() - g64).abs().max()), 2.0 ** -24 * top)
            for k, v in want['loss_dict'].items():
                if dtype == torch.float64:
                    assert _close(loss_dict[k], v, 1e-12), (source, k)
                elif same_machine:
                    assert torch.equal(loss_dict[k].detach(), v), (source, k)     # bit for bit
                else:
                    v64 = float(want64['loss_dict'][k])
                    assert abs(float(loss_dict[k].detach()) - v64) <= 4 * max(abs(float(v) - v64), 2.0 ** -24 * abs(v64)), (source, k)
    if here:                                                           # the recorded file is what the reference gives
        for k, v in here['runs'][(flags, 'fp64')]['loss_dict'].items():
            assert _close(v, fix['runs'][(flags, 'fp64')]['loss_dict'][k], 1e-12), k


@pytest.mark.parametrize('with_global', [True, False])
def test_row_layout_of_the_batch(with_global):
    """the stacked rows are the reference's own query rows, block by block, bit for bit"""
    data = tc.synthetic_data(48, 32, 4, seed=1)
    idx = tc.sample(data, 257, seed=2, corners=True)
    d, D = 1, 100
    b = tc.batch_restated(idx, data, d, D, with_global)
    q = tc.Queries.from_data(tc.jif_of(idx, 32, 48), data, d, D)
    B = 9 if with_global else 7
    assert b['rows'].shape == (B, 257, 3) and b['rows'].dtype == torch.float32
    for block in (0, 1, 2):
        assert torch.equal(b['rows'][block], q.rows(block))
    assert torch.equal(torch.cat((b['rows'][3], b['rows'][4])), q.rows((3, 4)))
    if with_global:
        assert torch.equal(torch.cat((b['rows'][5], b['rows'][6])), q.rows((5, 6)))
    assert torch.equal(b['rows'][B - 2][q.rel_f], q.rows(7)) and torch.equal(b['rows'][B - 1][q.rel_b], q.rows(8))
    assert torch.equal(torch.where(b['m_fwd'])[0], q.rel_f) and torch.equal(torch.where(b['m_bwd'])[0], q.rel_b)
    assert b['counts'].tolist() == [q.rel_f.numel(), q.rel_b.numel()] and 0 < q.rel_f.numel() < 257
    assert torch.equal(b['rgb'], q.rgb) and torch.equal(b['rgb_dx'], q.rgb_dx) and torch.equal(b['alpha_gt'].unsqueeze(-1), q.alpha_gt)
    # offsets that leave the image are coordinates only: the corner rows are there and finite
    assert bool(torch.isfinite(b['rows']).all()) and float(b['rows'][:, :8, :2].min()) < -1.0


def _toy(seed=3):
    models, data = tc.toy_training_set(seed)
    return {k: models[k] for k in NETS}, models['FG_UV_Mapping_Inverse'], data


@pytest.mark.parametrize('step,blocks', [(0, 9), (11, 7)])
def test_which_network_sees_which_block_and_once(step, blocks):
    from videoswap_amd import atlas_fit, ops
    models, _, data = _toy()
    N = 65
    idx = tc.sample(data, N, seed=step)
    seen = {}
    with tc.train_standin() as s:
        for k, m in models.items():
            m.differentiable_(True)
            m.register_forward_pre_hook(lambda mod, args, k=k: seen.setdefault(k, []).append(args[0].detach().clone()))
        b = ops.atlas_batch(idx, data, 1, 8, with_global_rigidity=blocks == 9)
        with counted('coord_mlp_train_forward', 'coord_mlp_backward', 'hash_mlp_train_forward', 'hash_mlp_backward') as box:
            total, loss_dict = atlas_fit.training_losses(models, b, tc.FIT_TRAIN, step)
            total.backward()
        assert box['calls'] == 8 and s.loss_calls == 1                 # each network once forward and once backward
    rows = b['rows']
    assert [len(v) for v in seen.values()] == [1] * 4
    assert torch.equal(seen['FG_UV_Mapping'][0], rows.view(-1, 3)) and torch.equal(seen['BG_UV_Mapping'][0], rows.view(-1, 3))
    assert torch.equal(seen['F_Alpha'][0], torch.cat((rows[0], rows[1], rows[2], rows[blocks - 2], rows[blocks - 1])))
    assert seen['F_Atlas'][0].shape == (6 * N, 2)
    keys = ['gradient_loss', 'rgb_loss', 'alpha_loss', 'alpha_mean_fg', 'alpha_mean_bg', 'sparsity_loss', 'rigidity_loss_fg', 'rigidity_loss_bg']
    keys += ['global_rigidity_loss_fg', 'global_rigidity_loss_bg'] if blocks == 9 else []
    keys += ['flow_loss_fg', 'flow_loss_bg', 'flow_alpha_loss', 'total_loss']
    assert list(loss_dict) == keys                                     # the reference's keys, in its order
    assert all(v.dim() == 0 for v in loss_dict.values()) and loss_dict['total_loss'] is total
    no_alpha = dict(tc.FIT_TRAIN, pretrain_alpha_iter=-1)
    with tc.train_standin():
        assert 'alpha_loss' not in atlas_fit.training_losses(models, b, no_alpha, step)[1]
        with pytest.raises(ValueError, match='blocks'):
            atlas_fit.training_losses(models, b, tc.FIT_TRAIN, 11 if blocks == 9 else 0)


@pytest.mark.parametrize('N,step', [(65, 0), (257, 11)])
def test_stacked_step_gives_the_block_by_block_gradients(N, step):
    """every parameter gradient of training_losses (each network ONCE, on stacked rows, one loss Function) against the fp64
    restatement that calls the networks block by block and compacts the flow rows, under the 4x rule"""
    from videoswap_amd import atlas_fit, ops
    models, _, data = _toy(seed=5)
    idx, dropped = tc.select_pixels(models, data, tc.FIT_TRAIN, N, seed=N, with_global=step <= tc.FIT['global_until'])
    g64, L64 = tc.step_param_grads(models, idx, data, tc.FIT_TRAIN, step, torch.float64)
    g32, L32 = tc.step_param_grads(models, idx, data, tc.FIT_TRAIN, step, torch.float32)
    with tc.train_standin():
        nets = {k: copy.deepcopy(m).differentiable_(True) for k, m in models.items()}
        b = ops.atlas_batch(idx, data, 1, 8, with_global_rigidity=step <= tc.FIT['global_until'])
        total, loss_dict = atlas_fit.training_losses(nets, b, tc.FIT_TRAIN, step)
        total.backward()
    import hash_fit_case as hc
    e32, e = hc.worst_error(g32, g64), hc.worst_error(tc.module_grads(nets), g64)
    print(f'step N={N}: E stand-in {e:.3e}, E fp32 torch {e32:.3e}, dropped {dropped:.3f}')
    assert e <= 4 * e32
    assert abs(float(total.detach()) - float(L64[11])) <= max(4 * abs(float(L32[11]) - float(L64[11])), 1e-6 * abs(float(L64[11])))


def _k18b_case(N, seed, with_global=True, with_alpha=True, masks='data'):
    data = tc.synthetic_data(48, 32, 4, seed=seed)
    batch = tc.with_masks(tc.batch_restated(tc.sample(data, N, seed, corners=True), data, 1, 100, with_global), masks)
    outs = tc.synthetic_outputs(N, batch, tc.TRAIN, seed)
    return batch, outs[:4], tc.flat_cfg(tc.TRAIN, with_alpha), outs[4]


@pytest.mark.parametrize('masks', ['none', 'one', 'all'])
def test_flow_terms_without_a_relevant_row_are_zero(masks):
    batch, outs, cfg, _ = _k18b_case(65, 3, masks=masks)
    for dtype in (torch.float64, torch.float32):
        L, g_fg, g_bg, g_a, g_rgb = tc.losses_from_outputs(*outs, batch, cfg, dtype)
        assert bool(torch.isfinite(L).all())
        flows = [float(L[tc.LOSSES.index(k)]) for k in ('flow_loss_fg', 'flow_loss_bg', 'flow_alpha_loss')]
        if masks == 'none':
            assert flows == [0.0, 0.0, 0.0]
            assert not bool(g_fg.view(9, 65, 2)[7:].any()) and not bool(g_a.view(5, 65)[3:].any())   # a zero gradient for the matches
        else:
            assert all(v > 0 for v in flows)
            rel = batch['m_fwd'] != 0
            assert not bool(g_fg.view(9, 65, 2)[7][~rel].any()) and bool(g_fg.view(9, 65, 2)[7][rel].any())


def test_kink_exclusion_stays_far_inside_its_cap():
    for N in tc.NS[1:]:
        for seed in range(4):
            assert _k18b_case(N, 100 * N + seed)[3] <= 0.01            # the cap is 0.05 (asserted inside)


# A swapped du_dy / dv_dx transposes the Jacobian, and the rigidity loss is a function of the singular values of J alone
# (|JtJ|_F and |(JtJ + 0.001 I)^-1|_F): J^T has the same ones, so the swap changes neither the value nor, by symmetry, the
# gradient with respect to uv.  No rule can catch it; what a test CAN show is this invariance (below).
CATCHABLE = tuple(p for p in tc.PLANTS if p != 'swap_jacobian')


def test_a_transposed_jacobian_is_invisible_to_the_rigidity_loss():
    batch, outs, cfg, _ = _k18b_case(257, 9)
    want64 = tc.losses_from_outputs(*outs, batch, cfg, torch.float64)
    swapped64 = tc.losses_from_outputs(*outs, batch, cfg, torch.float64, plant='swap_jacobian')
    assert tc.grad_error(swapped64[1:], want64[1:]) < 1e-12
    assert float((swapped64[0][:12] - want64[0][:12]).abs().max()) <= 1e-12 * float(want64[0][11])


@pytest.mark.parametrize('plant', CATCHABLE)
def test_the_rules_catch_planted_errors(plant):
    """each planted error breaks the gradient rule by more than an order of magnitude"""
    batch, outs, cfg, _ = _k18b_case(257, 9)
    want64 = tc.losses_from_outputs(*outs, batch, cfg, torch.float64)
    want32 = tc.losses_from_outputs(*outs, batch, cfg, torch.float32)
    e32 = tc.grad_error(want32[1:], want64[1:])
    good = tc.TrainStandin().atlas_losses(*outs, batch, cfg)
    bad = tc.TrainStandin(plant).atlas_losses(*outs, batch, cfg)
    e_good, e_bad = tc.grad_error(good[1:], want64[1:]), tc.grad_error(bad[1:], want64[1:])
    print(f'{plant}: E fp32 torch {e32:.3e}, E stand-in {e_good:.3e}, E planted {e_bad:.3e}')
    assert e_good <= 4 * e32 and not tc.values_within_rule(good[0], want32[0], want64[0], 257)
    assert e_bad > 10 * (4 * e32)


def test_refusals():
    from videoswap_amd import atlas_fit, ops
    from videoswap_amd._lib import VsxError
    models, inverse, data = _toy()
    with tc.train_standin():
        with pytest.raises(VsxError, match='idx outside'):
            ops.atlas_batch(torch.tensor([[48 * 32 * 4]]), data, 1, 8)
        with pytest.raises(VsxError, match='idx outside'):
            ops.atlas_batch(torch.tensor([[-1]]), data, 1, 8)
        two_levels = dict(data, optical_flows=torch.zeros(32, 48, 2, 4, 2))
        with pytest.raises(NotImplementedError, match='flow levels'):
            ops.atlas_batch(torch.tensor([[0]]), two_levels, 1, 8)
        with pytest.raises(NotImplementedError, match='optimizer'):
            atlas_fit.fit_atlas(models, data, dict(tc.FIT_TRAIN, optimizer={'type': 'SGD', 'lr': 1e-3}), 1, batch=8)


def test_fit_atlas_follows_its_fp64_restatement_on_the_cpu():
    models, data = tc.toy_training_set(pretrained=True)
    before = {k: copy.deepcopy(m.state_dict()) for k, m in models.items()}
    with tc.train_standin() as s:
        hist, last, nets = tc.run_fit(models, data, 'cpu')
    assert s.batch_calls == s.loss_calls == tc.FIT['iters'] and len(hist) == tc.FIT['iters']
    h64, inv64 = tc.fit_fp64(models, data)
    assert all(torch.equal(v, before[k][n]) for k, m in models.items() for n, v in m.state_dict().items())    # copies were trained
    assert all(not torch.equal(v, before[k][n]) for k, m in nets.items() for n, v in m.state_dict().items() if v.numel() > 3)
    d = tc.history_diff(hist, h64)
    print(f'fit_atlas: total_loss {hist[0]:.4f} -> {hist[-1]:.4f}; vs fp64 {d:.3e}; fg_inv_loss {last["fg_inv_loss"]:.6f} vs {inv64[-1]:.6f}')
    assert hist[-1] < hist[0] and d <= 1e-4 * abs(h64[0])
    assert abs(last['fg_inv_loss'] - inv64[-1]) <= 1e-4 * inv64[-1]
    assert set(last) >= {'total_loss', 'flow_loss_fg', 'fg_inv_loss'} and 'global_rigidity_loss_fg' not in last     # global rigidity ended at step 10
    assert not any(m._differentiable for m in nets.values())           # the switch is back where it was


# ------------------------------------------------------------------------------------------------
# load_training_data and the train_atlas command
# ------------------------------------------------------------------------------------------------
def _write_dataset(root, W=12, H=8, T=3, seed=0):
    import numpy as np
    from PIL import Image
    rng = np.random.default_rng(seed)
    for sub in ('frames', 'masks', 'flows'):
        (root / sub).mkdir()
    frames = rng.integers(0, 256, size=(T, H, W, 3), dtype=np.uint8)
    masks = (rng.random((T, H, W)) < 0.5).astype(np.uint8) * 255
    flows = []
    for f in range(T):
        Image.fromarray(frames[f]).save(root / 'frames' / f'{f:05d}.png')
        Image.fromarray(masks[f]).save(root / 'masks' / f'{f:05d}.png')
        if f < T - 1:
            shift = rng.uniform(-1.5, 1.5, size=2)
            fwd = (shift + rng.normal(0, 0.4, size=(H, W, 2))).astype(np.float32)
            bwd = (-shift + rng.normal(0, 0.4, size=(H, W, 2))).astype(np.float32)
            flows.append(np.stack((fwd, bwd)))
            np.save(root / 'flows' / f'{f:05d}.npy', flows[-1])
    opt = dict(frame_path=str(root / 'frames'), mask_path=str(root / 'masks'), flow_path=str(root / 'flows'), res_x=W, res_y=H,
               max_frames=T, filter_optical_flow=True, sample_batch_size=64)
    return opt, frames, masks, flows


def _brute_force_mask(f12, f21):
    """|f12 + f21 sampled bilinearly at x + f12| < 1, pixel by pixel in double precision, zero outside the image"""
    import math
    H, W = f12.shape[:2]
    out = torch.zeros(H, W)
    for y in range(H):
        for x in range(W):
            px, py = x + float(f12[y, x, 0]), y + float(f12[y, x, 1])
            x0, y0 = math.floor(px), math.floor(py)
            acc = [0.0, 0.0]
            for yy, wy in ((y0, 1 - (py - y0)), (y0 + 1, py - y0)):
                for xx, wx in ((x0, 1 - (px - x0)), (x0 + 1, px - x0)):
                    if 0 <= xx < W and 0 <= yy < H:
                        acc[0] += wx * wy * float(f21[yy, xx, 0])
                        acc[1] += wx * wy * float(f21[yy, xx, 1])
            out[y, x] = float(math.hypot(float(f12[y, x, 0]) + acc[0], float(f12[y, x, 1]) + acc[1]) < 1.0)
    return out


def test_load_training_data_on_a_synthetic_directory(tmp_path):
    import numpy as np
    from videoswap_amd import atlas_fit, ops
    opt, frames, masks, flows = _write_dataset(tmp_path)
    data = atlas_fit.load_training_data(opt)
    W, H, T = 12, 8, 3
    assert set(data) == set(ops.ATLAS_DATA_KEYS) and all(v.dtype == torch.float32 for v in data.values())
    assert data['video_frames'].shape == (H, W, 3, T) and data['mask_frames'].shape == (H, W, T)
    assert data['optical_flows'].shape == (H, W, 2, T, 1) and data['optical_flows_mask'].shape == (H, W, T, 1)
    video = torch.from_numpy(frames.astype(np.float32) / 255.0).permute(1, 2, 3, 0)
    assert torch.equal(data['video_frames'], video) and torch.equal(data['mask_frames'], torch.from_numpy(masks / 255.0).float().permute(1, 2, 0))
    dx, dy = torch.zeros_like(video), torch.zeros_like(video)
    dy[:-1], dx[:, :-1] = video[1:] - video[:-1], video[:, 1:] - video[:, :-1]
    assert torch.equal(data['video_frames_dx'], dx) and torch.equal(data['video_frames_dy'], dy)
    mixed = 0
    for f in range(T - 1):
        assert torch.equal(data['optical_flows'][:, :, :, f, 0], torch.from_numpy(flows[f][0]))
        assert torch.equal(data['optical_flows_reverse'][:, :, :, f + 1, 0], torch.from_numpy(flows[f][1]))
        want_f, want_b = _brute_force_mask(flows[f][0], flows[f][1]), _brute_force_mask(flows[f][1], flows[f][0])
        assert torch.equal(data['optical_flows_mask'][:, :, f, 0], want_f) and torch.equal(data['optical_flows_reverse_mask'][:, :, f + 1, 0], want_b)
        mixed += int(0 < want_f.sum() < H * W)
    assert mixed == T - 1                                              # both answers occur: the comparison says something
    assert not bool(data['optical_flows'][:, :, :, T - 1].any()) and not bool(data['optical_flows_reverse_mask'][:, :, 0].any())
    unfiltered = atlas_fit.load_training_data(dict(opt, filter_optical_flow=False))
    assert bool((unfiltered['optical_flows_mask'][:, :, :T - 1] == 1).all()) and bool((unfiltered['optical_flows_reverse_mask'][:, :, 1:] == 1).all())
    with pytest.raises(ImportError, match='cv2'):                      # flows at another resolution need cv2
        atlas_fit.load_training_data(dict(opt, res_x=6, res_y=4))
    (tmp_path / 'flows' / '00001.npy').unlink()
    with pytest.raises(FileNotFoundError, match='flow files'):
        atlas_fit.load_training_data(opt)


def test_train_atlas_command_writes_a_checkpoint_the_tools_read(tmp_path):
    import yaml
    import atlas_render_case as arc
    from videoswap_amd import atlas, train_atlas
    data_root = tmp_path / 'data'
    data_root.mkdir()
    datasets, _, _, _ = _write_dataset(data_root)
    opt = {'name': 'toy_atlas', 'manual_seed': 0, 'mixed_precision': 'no', 'datasets': datasets, 'models': arc.toy_config(hidden=32),
           'train': dict(tc.TRAIN, total_iter=3, pretrain_UV_mapping_iter=1, global_derivative_amount=3, pretrain_global_rigidity_iter=1),
           'val': {'val_freq': 2}, 'logger': {'print_freq': 1, 'save_checkpoint_freq': 2}}
    cfg = tmp_path / 'toy_atlas.yml'
    cfg.write_text(yaml.safe_dump(opt))
    lines = []
    with tc.train_standin() as s:
        out = train_atlas.run(train_atlas.build_parser().parse_args(['-opt', str(cfg), '--root', str(tmp_path / 'experiments')]), device='cpu',
                              log=lines.append)
        assert s.loss_calls == 3 and len(out['history']) == 3
        assert [os.path.basename(p) for p in out['checkpoints']] == ['models_2.pth', 'models_3.pth'] and all(os.path.isfile(p) for p in out['checkpoints'])
        ckpt = torch.load(out['checkpoints'][-1], map_location='cpu', weights_only=True)
        assert set(ckpt) == {'F_Atlas', 'FG_UV_Mapping', 'BG_UV_Mapping', 'F_Alpha', 'FG_UV_Mapping_Inverse'}
        models = atlas.load_atlas_models(str(cfg), out['checkpoints'][-1], names=atlas.RENDER_MODEL_NAMES)
        frames = atlas.render_atlas(models, 12, 8, 3)['reconstruction']
    assert frames.shape == (3, 8, 12, 3) and bool(torch.isfinite(frames).all())
    text = '\n'.join(lines)
    assert text.count('Finish pretrain') == 2 and text.count('[iter ') == 3 and 'Validation Reconstruction PSNR' in text and 'fg_inv_loss' in text
