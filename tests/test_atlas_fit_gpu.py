"""Weight and bias gradients of the coordinate MLP (csrc/atlas_bwd.hip, K16) and the two fits built on them, on the MI355X.

Gradient parity (the helper atlas_fit_case.py holds the cases, the fp64 reference, the input selection and the rule): per
parameter tensor e = max |g - g64| / max |g64|, E = the largest e of a case, and E_kernel <= 4 E_fp32torch on the same
inputs.  Both figures of every case are printed; VSX_WRITE_PROFILES=1 writes profiles/atlas_fit_parity.json.

pretrain_mapping runs against the reference's own run (tests/golden/atlas_pretrain.pt), fit_inverse_mapping against an fp64
restatement on the CPU, both under the same 4 x rule.
"""
import json
import os

import pytest
import torch

import atlas_fit_case as case
from atlas_case import counted, swapped
from util import ROOT

pytestmark = pytest.mark.gpu

_parity = []
_NET = dict(input_dim=3, output_dim=2, hidden_dim=64, mlp_layers=4)


@pytest.mark.parametrize('name,kw,N,scale', case.RUNS, ids=case.RUN_IDS)
def test_gradients_against_fp64(name, kw, N, scale):
    m = case.network(kw, scale, seed=N % 1000 + len(name))
    x, dropped, delta = case.select_inputs(m, N, seed=N)             # on the CPU, from the references alone
    G = case.cotangent(N, kw['output_dim'], seed=N)
    g64, g32 = case.reference_grads(m, x, G, torch.float64), case.reference_grads(m, x, G, torch.float32)
    m = m.cuda()
    with torch.no_grad():
        y_plain = m(x.cuda()).cpu()
    y, grads = case.backward_through(m.differentiable_(True), x, G)
    assert torch.equal(y, y_plain)                                   # the training forward gives the plain forward's bits
    _, again = case.backward_through(m, x, G)
    assert all(torch.equal(a, b) for a, b in zip(grads, again))      # no atomics, a fixed order: the same bits twice
    assert all(bool(torch.isfinite(g).all()) for g in grads)
    e_torch, e_kernel = case.worst_error(g32, g64), case.worst_error(grads, g64)
    print(f'coord_mlp gradients {name} N={N} scale={scale}: E fp32 torch {e_torch:.3e}, E kernel {e_kernel:.3e}, '
          f'dropped candidates {dropped:.3f}, delta {delta:.2e}')
    _parity.append({'case': name, 'N': N, 'weight_scale': scale, 'E_fp32_torch': e_torch, 'E_kernel': e_kernel, 'bound': 4 * e_torch,
                    'dropped_share': dropped})
    assert e_kernel <= 4 * e_torch, (e_kernel, e_torch)


def test_parity_figures_recorded():
    """runs after the parity cases (file order): all of them left a figure; VSX_WRITE_PROFILES=1 writes the profile"""
    assert len(_parity) == len(case.RUNS)
    if os.environ.get('VSX_WRITE_PROFILES') == '1':
        out = os.environ.get('VSX_PROFILE_DIR', os.path.join(ROOT, 'profiles'))
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, 'atlas_fit_parity.json'), 'w') as f:
            json.dump({'device': torch.cuda.get_device_name(0),
                       'rule': 'E = max over parameter tensors of max|g - g64| / max|g64|; E_kernel <= 4 * E_fp32_torch',
                       'cases': _parity}, f, indent=1)


def test_no_rows_give_zero_gradients():
    m = case.network(case.FG, 1.0, seed=1).cuda().differentiable_(True)
    y, grads = case.backward_through(m, torch.zeros(0, 3), torch.zeros(0, 2))
    assert y.shape == (0, 2)
    for q, g in zip(m.parameters(), grads):
        assert g.shape == q.shape and not bool(g.any())


def test_ops_calls_do_not_depend_on_the_rows():
    m = case.network(case.FG, 1.0, seed=2).cuda().differentiable_(True)
    calls = []
    for N in (8, 5000):
        x, G = torch.rand(N, 3) * 2 - 1, case.cotangent(N, 2, seed=N)
        with counted('coord_mlp', 'coord_mlp_train_forward', 'coord_mlp_backward', 'coord_mlp_train_workspace') as box:
            case.backward_through(m, x, G)
        calls.append(box['calls'])
    assert calls == [2, 2]                                           # one forward call, one backward call


def test_refusals():
    from videoswap_amd import ops
    from videoswap_amd._lib import VsxError
    m = case.network(_NET, 1.0, seed=3).cuda()
    x = (torch.rand(100, 3) * 2 - 1).cuda()
    n_saved, _, n_grad = ops.coord_mlp_train_workspace(100, **_NET)
    out, saved = ops.coord_mlp_train_forward(x, m.packed(), **_NET)
    assert saved.numel() == n_saved
    gout = torch.ones_like(out)
    assert ops.coord_mlp_backward(gout, saved, m.packed(), **_NET).numel() == n_grad
    with pytest.raises(VsxError, match='saved'):
        ops.coord_mlp_train_forward(x, m.packed(), **_NET, saved=torch.empty(n_saved - 1, device='cuda'))
    with pytest.raises(VsxError, match='saved'):
        ops.coord_mlp_backward(gout, saved[:-1], m.packed(), **_NET)
    short = torch.full((n_grad - 1,), 7.0, device='cuda')
    with pytest.raises(VsxError, match='grad'):
        ops.coord_mlp_backward(gout, saved, m.packed(), **_NET, grad=short)
    assert bool((short == 7.0).all())                                # refused before anything was written
    with pytest.raises(NotImplementedError, match='input gradients'):
        m.differentiable_(True)(x.clone().requires_grad_(True))
    w = torch.zeros(64, device='cuda')
    for kw, word in ((dict(pe_type='hash_encoding'), 'hash_encoding'), (dict(mlp_type='tcnn'), 'tcnn'),
                     (dict(hidden_dim=48), 'hidden_dim'), (dict(hidden_dim=512), 'hidden_dim'), (dict(mlp_layers=9), 'mlp_layers'),
                     (dict(mlp_layers=1), 'mlp_layers'), (dict(output_dim=4), 'output_dim'), (dict(skip_layers=[0]), 'skip_layers'),
                     (dict(pe_type='encoding', pe_dim=11), 'pe_dim')):
        args = dict(_NET)
        args.update(kw)
        with pytest.raises(NotImplementedError, match=word):
            ops.coord_mlp_train_forward(x, w, **args)
        with pytest.raises(NotImplementedError, match=word):
            ops.coord_mlp_backward(torch.ones(100, args['output_dim'], device='cuda'), saved, w, **args)


def test_flag_off_is_the_plain_forward():
    m = case.network(_NET, 1.0, seed=4).cuda()                       # training mode, parameters require grad, grad mode on
    x = (torch.rand(33, 3) * 2 - 1).cuda()
    seen = []

    def forbidden(*a, **k):
        raise AssertionError('the gradient path ran with differentiable_ off')

    from videoswap_amd import ops
    plain = ops._raw['coord_mlp']
    with swapped(coord_mlp=lambda *a, **k: (seen.append((a[2:], k)), plain(*a, **k))[1], coord_mlp_train_forward=forbidden):
        y = m(x)
    assert y.grad_fn is None and not y.requires_grad and len(seen) == 1
    assert seen[0] == ((3, 2, 64, 4), dict(pe_type='none', pe_dim=10, mlp_type='origin', skip_layers=[], use_tanh=True))


def test_pretrain_mapping_follows_the_reference():
    case.check_pretrain_fixture('cuda')


def test_inverse_fit_follows_the_fp64_restatement():
    nets = case.fit_networks()
    h64 = case.fit_fp64(nets)
    with case.fit_standin():
        h32 = case.run_fit(nets, 'cpu')['loss_history']
    res = case.run_fit(nets, 'cuda')
    hist = res['loss_history']
    d_kernel, d_standin = case.history_diff(hist, h64), case.history_diff(h32, h64)
    print(f'inverse fit: loss {hist[0]:.6f} -> {hist[-1]:.6f}; vs fp64: kernel {d_kernel:.3e}, fp32 stand-in {d_standin:.3e}; '
          f'round trip {res["roundtrip_mean_px"]:.2f} / {res["roundtrip_max_px"]:.2f} px on {res["holdout_rows"]} rows')
    assert res['steps_skipped'] == 0 and hist[-1] < hist[0]
    assert d_kernel <= 4 * d_standin, (d_kernel, d_standin)


def test_a_batch_without_foreground_is_skipped():
    res = case.run_fit(case.fit_networks(alpha_shift=-50.0), 'cuda', iters=2)
    assert res['loss_history'] == [] and res['steps_skipped'] == 2 and res['holdout_rows'] == 0
