"""The gradients of the hash-grid texture network (csrc/atlas_bwd.hip K17, the training forward in csrc/atlas.hip) and
atlas.fit_reconstruction, on the MI355X.

Gradient parity (the helper hash_fit_case.py holds the differentiable restatement, the fp64 and fp32 references, the input
selection and the rule): per tensor (every layer's weight and bias gradient, the table gradient, grad_x)
e = max |g - g64| / max |g64|, E = the largest e of a case, and E_kernel <= 4 E_fp32torch on the same inputs.  The layer
gradients and grad_x are bit-equal across two calls; the table gradient (fp32 atomics) is not required to be, and BOTH
calls' table gradients stand under the rule.  Every case prints E_kernel, E_fp32torch and the dropped share;
VSX_WRITE_PROFILES=1 writes profiles/hash_fit_parity.json.

Measured on the MI355X (profiles/hash_fit_parity.json): see DESIGN.md §14.
"""
import json
import os

import pytest
import torch

import hash_fit_case as hc
from atlas_case import counted
from util import ROOT

pytestmark = pytest.mark.gpu

NS = (1, 63, 64, 65, 513, 2000)
# stacks x grids x N x {default initialisation, 2 x}
RUNS = [(s, g, n, w, False) for s in hc.STACKS for g in hc.GRIDS for n in NS for w in (1.0, 2.0)]
# 1000 rows inside one finest-level cell: every add of a level lands on four addresses
RUNS += [('real', 'g16-scaled', 1000, 1.0, True), ('h64', 'small-half', 1000, 2.0, True)]
# once the reference's own grid at its initialisation: offsets past 2^19 entries
RUNS += [('real', 'reference-tiny', 1000, 1.0, False)]
RUN_IDS = [f'{s}-{g}-{n}-x{w:g}' + ('-onecell' if c else '') for s, g, n, w, c in RUNS]
_parity = []


def _grid(name):
    if name == 'reference-tiny':
        from videoswap_amd.atlas import HASH_GRID
        return HASH_GRID, 'tiny'
    return hc.GRIDS[name]


def _case(stack, grid, N, scale, one_cell):
    """the network, its selected inputs and both references, on the CPU from the references alone"""
    cfg, family = _grid(grid)
    seed = N % 1000 + len(stack) + 7 * len(grid)
    m = hc.network(hc.STACKS[stack], cfg, family, scale, seed)
    x, dropped, delta = hc.select_inputs(m, N, seed=N, one_cell=one_cell)
    G = hc.cotangent(N, m.output_dim, seed=N)
    return m, x, G, dropped, hc.reference_grads(m, x, G, torch.float64), hc.reference_grads(m, x, G, torch.float32)


@pytest.mark.parametrize('stack,grid,N,scale,one_cell', RUNS, ids=RUN_IDS)
def test_gradients_against_fp64(stack, grid, N, scale, one_cell):
    m, x, G, dropped, g64, g32 = _case(stack, grid, N, scale, one_cell)
    m = m.cuda()
    with torch.no_grad():
        y_plain = m(x.cuda()).cpu()
    y, grads = hc.backward_through(m.differentiable_(True), x, G)
    assert torch.equal(y, y_plain)                                   # the training forward gives the plain forward's bits
    _, again = hc.backward_through(m, x, G)
    table, table2 = grads[-2], again[-2]
    for a, b in zip(grads[:-2] + grads[-1:], again[:-2] + again[-1:]):
        assert torch.equal(a, b)                                     # layers and grad_x: no atomics, the same bits twice
    assert all(bool(torch.isfinite(g).all()) for g in grads + again)
    untouched = ~hc.addressed(m, x)
    assert not bool(table[untouched].any()) and not bool(table2[untouched].any())   # exactly zero where no corner lands
    e_torch = hc.worst_error(g32, g64)
    e_kernel = max(hc.worst_error(grads, g64), hc.worst_error(again, g64))
    print(f'hash_mlp gradients {stack} {grid} N={N} scale={scale} one_cell={one_cell}: E fp32 torch {e_torch:.3e}, '
          f'E kernel {e_kernel:.3e}, dropped candidates {dropped:.3f}, table bit-equal twice {torch.equal(table, table2)}')
    _parity.append({'stack': stack, 'grid': grid, 'N': N, 'weight_scale': scale, 'one_cell': one_cell, 'E_fp32_torch': e_torch,
                    'E_kernel': e_kernel, 'bound': 4 * e_torch, 'dropped_share': dropped})
    assert e_kernel <= 4 * e_torch, (e_kernel, e_torch)


def test_parity_figures_recorded():
    """runs after the parity cases (file order): all of them left a figure; VSX_WRITE_PROFILES=1 writes the profile"""
    assert len(_parity) == len(RUNS)
    if os.environ.get('VSX_WRITE_PROFILES') == '1':
        out = os.environ.get('VSX_PROFILE_DIR', os.path.join(ROOT, 'profiles'))
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, 'hash_fit_parity.json'), 'w') as f:
            json.dump({'device': torch.cuda.get_device_name(0),
                       'rule': 'E = max over the layer, table and input gradients of max|g - g64| / max|g64|; E_kernel <= 4 * E_fp32_torch',
                       'cases': _parity}, f, indent=1)


@pytest.mark.parametrize('grid', list(hc.GRIDS))
def test_grid_backward_alone_against_the_restatement(grid):
    from videoswap_amd import ops
    cfg, family = hc.GRIDS[grid]
    m = hc.network(hc.H32, cfg, family, 1.0, seed=11)
    E = 2 * cfg['n_levels']
    for N in (1, 65, 513):
        gen = torch.Generator().manual_seed(N)
        x, ge = torch.rand(N, 2, generator=gen) * 2 - 1, torch.randn(N, E, generator=gen) / N
        want = {}
        for dtype in (torch.float64, torch.float32):
            xd, td = x.to(dtype).requires_grad_(True), m.encoder.params.detach().to(dtype).requires_grad_(True)
            want[dtype] = list(torch.autograd.grad((hc.hash_encode_diff(xd, td, cfg, dtype) * ge.to(dtype)).sum(), [td, xd]))
        table = m.encoder.params.detach().cuda()
        gt, gx = ops.hash_grid_backward(x.cuda(), ge.cuda(), table, cfg)
        gt_only, none = ops.hash_grid_backward(x.cuda(), ge.cuda(), table, cfg, want_x=False)
        none2, gx_only = ops.hash_grid_backward(x.cuda(), ge.cuda(), table, cfg, want_table=False)
        assert none is None and none2 is None and torch.equal(gx, gx_only)
        e_torch = hc.worst_error(want[torch.float32], want[torch.float64])
        e_kernel = max(hc.worst_error([gt.cpu(), gx.cpu()], want[torch.float64]), hc.worst_error([gt_only.cpu(), gx.cpu()], want[torch.float64]))
        print(f'hash_grid_backward {grid} N={N}: E fp32 torch {e_torch:.3e}, E kernel {e_kernel:.3e}')
        assert e_kernel <= 4 * e_torch, (e_kernel, e_torch)
        assert not bool(gt.cpu()[~hc.addressed(m, x)].any())


def test_no_rows_give_zero_gradients():
    from videoswap_amd import ops
    m = hc.network(hc.H64, hc.SMALL_GRID, 'half', 1.0, seed=1).cuda().differentiable_(True)
    y, grads = hc.backward_through(m, torch.zeros(0, 2), torch.zeros(0, 3))
    assert y.shape == (0, 3) and grads[-1].shape == (0, 2)
    for q, g in zip(list(m.hidden.parameters()) + [m.encoder.params], grads[:-1]):
        assert g.shape == q.shape and not bool(g.any())
    gt, gx = ops.hash_grid_backward(torch.zeros(0, 2, device='cuda'), torch.zeros(0, 8, device='cuda'), m.encoder.params.detach(), m.grid)
    assert gx.shape == (0, 2) and not bool(gt.any())


def test_ops_calls_do_not_depend_on_the_rows():
    m = hc.network(hc.H64, hc.SMALL_GRID, 'half', 1.0, seed=2).cuda().differentiable_(True)
    calls = []
    for N in (8, 5000):
        x, G = torch.rand(N, 2) * 2 - 1, hc.cotangent(N, 3, seed=N)
        with counted('hash_mlp', 'hash_grid', 'hash_grid_backward', 'hash_mlp_train_forward', 'hash_mlp_backward',
                     'hash_mlp_train_workspace') as box:
            hc.backward_through(m, x, G)
        calls.append(box['calls'])
    assert calls == [2, 2]                                           # one forward call, one backward call


def test_refusals():
    from videoswap_amd import ops
    from videoswap_amd._lib import VsxError
    net = dict(output_dim=3, hidden_dim=64, mlp_layers=4, skip_layers=[2])
    grid = hc.SMALL_GRID
    m = hc.network(hc.H64, grid, 'half', 1.0, seed=3).cuda()
    table = m.encoder.params.detach()
    x = (torch.rand(100, 2) * 2 - 1).cuda()
    n_saved, n_scratch, n_grad = ops.hash_mlp_train_workspace(100, grid, **net)
    out, saved = ops.hash_mlp_train_forward(x, table, grid, m.packed(), **net)
    assert saved.numel() == n_saved
    gout = torch.ones_like(out)
    grad, gt, gx = ops.hash_mlp_backward(gout, x, table, grid, saved, m.packed(), **net)
    assert grad.numel() == n_grad and gt.shape == table.shape and gx.shape == x.shape
    with pytest.raises(VsxError, match='saved'):
        ops.hash_mlp_train_forward(x, table, grid, m.packed(), **net, saved=torch.empty(n_saved - 1, device='cuda'))
    with pytest.raises(VsxError, match='saved'):
        ops.hash_mlp_backward(gout, x, table, grid, saved[:-1], m.packed(), **net)
    with pytest.raises(VsxError, match='scratch'):
        ops.hash_mlp_backward(gout, x, table, grid, saved, m.packed(), **net, scratch=torch.empty(n_scratch - 1, device='cuda'))
    short = torch.full((n_grad - 1,), 7.0, device='cuda')
    with pytest.raises(VsxError, match='grad'):
        ops.hash_mlp_backward(gout, x, table, grid, saved, m.packed(), **net, grad=short)
    assert bool((short == 7.0).all())                                # refused before anything was written
    for call in (lambda t: ops.hash_mlp_train_forward(x, t, grid, m.packed(), **net),
                 lambda t: ops.hash_mlp_backward(gout, x, t, grid, saved, m.packed(), **net),
                 lambda t: ops.hash_grid_backward(x, torch.ones(100, 8, device='cuda'), t, grid)):
        with pytest.raises(VsxError, match='grid table holds'):       # a table of another length
            call(torch.zeros(table.numel() + 16, device='cuda'))
    w = torch.zeros(64, device='cuda')
    for kw, word in ((dict(hidden_dim=48), 'hidden_dim'), (dict(hidden_dim=512), 'hidden_dim'), (dict(mlp_layers=9), 'mlp_layers'),
                     (dict(mlp_layers=1), 'mlp_layers'), (dict(output_dim=4), 'output_dim'), (dict(skip_layers=[0]), 'skip_layers')):
        args = dict(net)
        args.update(kw)
        with pytest.raises(NotImplementedError, match=word):
            ops.hash_mlp_train_forward(x, table, grid, w, **args)
        with pytest.raises(NotImplementedError, match=word):
            ops.hash_mlp_backward(torch.ones(100, args['output_dim'], device='cuda'), x, table, grid, saved, w, **args)
        with pytest.raises(NotImplementedError, match=word):
            ops.hash_mlp_train_workspace(100, grid, **args)
    for kw, word in ((dict(n_features_per_level=4), 'n_features_per_level'), (dict(n_levels=33), 'n_levels'),
                     (dict(log2_hashmap_size=25), 'log2_hashmap_size'), (dict(base_resolution=0), 'base_resolution'),
                     (dict(per_level_scale=0.5), 'per_level_scale')):
        bad = dict(grid, **kw)
        with pytest.raises(NotImplementedError, match=word):
            ops.hash_mlp_train_forward(x, table, bad, m.packed(), **net)
        with pytest.raises(NotImplementedError, match=word):
            ops.hash_mlp_backward(gout, x, table, bad, saved, m.packed(), **net)
        with pytest.raises(NotImplementedError, match=word):
            ops.hash_grid_backward(x, torch.ones(100, bad['n_levels'] * bad['n_features_per_level'], device='cuda'), table, bad)
        with pytest.raises(NotImplementedError, match=word):
            ops.hash_mlp_train_workspace(100, bad, **net)
    x3 = torch.zeros(100, 3, device='cuda')
    with pytest.raises(NotImplementedError, match='input_dim'):
        ops.hash_mlp_train_forward(x3, table, grid, m.packed(), **net)
    with pytest.raises(NotImplementedError, match='input_dim'):
        ops.hash_grid_backward(x3, torch.ones(100, 8, device='cuda'), table, grid)


def test_what_stays_refused():
    """CoordMLP keeps refusing input gradients and the coordinate training forward keeps refusing the hash encoding"""
    from videoswap_amd import ops
    from videoswap_amd.atlas import CoordMLP
    c = CoordMLP(3, 2, hidden_dim=32, mlp_layers=2).cuda().differentiable_(True)
    with pytest.raises(NotImplementedError, match='input gradients'):
        c(torch.zeros(4, 3, device='cuda', requires_grad=True))
    with pytest.raises(NotImplementedError, match='hash_encoding'):
        ops.coord_mlp_train_forward(torch.zeros(4, 2, device='cuda'), torch.zeros(64, device='cuda'), 2, 3, 32, 2, pe_type='hash_encoding')


def test_fit_reconstruction_follows_the_fp64_restatement():
    models, video, masks = hc.toy_atlas()
    h64 = hc.fit_fp64(models, video, masks)
    with hc.hash_fit_standin():
        h32, _ = hc.run_fit(models, video, masks, 'cpu')
    hist, _ = hc.run_fit(models, video, masks, 'cuda')
    d_kernel, d_standin = hc.history_diff(hist, h64), hc.history_diff(h32, h64)
    print(f'fit_reconstruction: loss {hist[0]:.6f} -> {hist[-1]:.6f}; vs fp64: kernel {d_kernel:.3e}, fp32 stand-in {d_standin:.3e}')
    assert hist[-1] < hist[0]
    assert d_kernel <= 4 * d_standin, (d_kernel, d_standin)
