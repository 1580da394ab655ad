"""Shared pieces of tests/test_hash_fit.py (CPU) and tests/test_hash_fit_gpu.py: a DIFFERENTIABLE torch restatement of the
hash grid of include/vsx.h K14 (atlas_render_case.hash_encode without detaching x or the table: the cell is chosen by
torch.floor on the fp32 position in both precisions, w = scale x + 0.5 - cell in `dtype`, so autograd differentiates one
bilinear patch in fp32 and in fp64), the networks, the fp64 and fp32 reference gradients, the input selection, the CPU
stand-ins of the four training ops of the hash-grid network (pure PyTorch, `saved` in the layout of include/vsx.h K17, with
planted errors for the tests of the rule's power), and the fp64 restatement of atlas.fit_reconstruction.

Reference: autograd of the restated grid and the F.linear chain of atlas_case.mlp_forward on the CPU (the skip input is a
DETACHED copy of the encoding), scalar (y * G).sum() for a fixed G ~ normal(0, 1) / N.

Input selection, as atlas_fit_case.select_inputs: of 2 N + 64 candidates uniform in [-1, 1)^2 every row with a hidden
pre-activation |z| < delta in fp64 is dropped, delta = 16 x the largest fp32-vs-fp64 pre-activation difference; the first N
survivors are used; at most half may be dropped (asserted: a condition, not a measurement).

Rule: per tensor e = max |g - g64| / max |g64| over every layer's weight and bias gradient, the table gradient and grad_x;
E = the largest e of a case; E_kernel <= 4 E_fp32torch on the same inputs (the project's margin for another summation
order, as in tests/test_atlas_fit_gpu.py).
"""
import contextlib

import torch
import torch.nn.functional as F

import atlas_case
import atlas_render_case
from atlas_case import mlp_forward, swapped, unpack
from atlas_fit_case import cotangent, worst_error  # noqa: F401  (re-exported to the tests)
from atlas_render_case import M32, SMALL_GRID

GRID16 = dict(n_levels=16, n_features_per_level=2, log2_hashmap_size=10, base_resolution=16, per_level_scale=1.38)
GRID20 = dict(n_levels=20, n_features_per_level=2, log2_hashmap_size=10, base_resolution=8, per_level_scale=1.2)

REAL = dict(input_dim=2, output_dim=3, hidden_dim=256, mlp_layers=8, skip_layers=[4, 7])
H64 = dict(REAL, hidden_dim=64, mlp_layers=4, skip_layers=[2])
H32 = dict(REAL, hidden_dim=32, mlp_layers=2, skip_layers=[])
NO_TANH = dict(H64, use_tanh=False, output_dim=2)
STACKS = {'real': REAL, 'h64': H64, 'h32': H32, 'no_tanh': NO_TANH}
# table families that stay within the selection's cap (it is asserted per case, on the CPU, from the references alone; the
# 16-level grid with +-0.5 at every level does not: its finest scale moves the features by 1e-4 and every row is dropped):
# 'half': uniform in +-0.5; 'tiny': +-1e-4 (tcnn's initialisation); 'scaled': level l uniform in +-0.5 scale_0 / scale_l
GRIDS = {'small-half': (SMALL_GRID, 'half'), 'g16-tiny': (GRID16, 'tiny'), 'g16-scaled': (GRID16, 'scaled'),
         'g20-scaled': (GRID20, 'scaled')}


def levels(cfg):
    from videoswap_amd.atlas import hash_grid_levels
    return hash_grid_levels(cfg)


def cells(x, cfg):
    """per level (lv, cell [N, 2] fp32, idx [4][N] int64 with the level's offset): the cell and corner entries of every row"""
    x32 = x.detach().to(torch.float32)
    out = []
    for lv in levels(cfg):
        cell = torch.floor(torch.tensor(lv['scale'], dtype=torch.float32) * x32 + 0.5)
        g = cell.to(torch.int64) & M32
        idx = []
        for c in range(4):
            c0, c1 = (g[:, 0] + (c & 1)) & M32, (g[:, 1] + (c >> 1)) & M32
            i = c0 ^ ((c1 * 2654435761) & M32) if lv['hashed'] else (c0 + c1 * lv['res']) & M32
            idx.append(i % lv['entries'] + lv['offset'])
        out.append((lv, cell, idx))
    return out


def hash_encode_diff(x, table, cfg, dtype):
    """atlas_render_case.hash_encode with x and the table left attached: x [N, 2] and table (flat) in `dtype`"""
    tab = table.view(-1, 2)
    cols = []
    for lv, cell, idx in cells(x, cfg):
        w = torch.tensor(lv['scale'], dtype=torch.float32).to(dtype) * x + 0.5 - cell.to(dtype)
        acc = torch.zeros(x.shape[0], 2, dtype=dtype)
        for c in range(4):
            weight = (w[:, 0] if c & 1 else 1 - w[:, 0]) * (w[:, 1] if c >> 1 else 1 - w[:, 1])
            acc = acc + weight.unsqueeze(1) * tab[idx[c]]
        cols.append(acc)
    return torch.cat(cols, dim=1)


def hash_forward_diff(weights, biases, table, cfg, x, skip_layers, use_tanh):
    """the network in the dtype of x, differentiable in everything; mlp_forward's `inp = x.clone()` is fed a detached copy
    through the skip layers exactly as IMLP_Hash.forward does (`input = x.detach().clone()`)"""
    enc = hash_encode_diff(x, table, cfg, x.dtype)
    inp, h = enc.detach().clone(), enc
    for i, (w, b) in enumerate(zip(weights, biases)):
        if i > 0:
            h = F.relu(h)
        if i in skip_layers:
            h = torch.cat((h, inp), 1)
        h = F.linear(h, w, b)
    return torch.tanh(h) if use_tanh else h


def fill_table(m, family, seed):
    g = torch.Generator().manual_seed(seed + 1000)
    with torch.no_grad():
        u = torch.rand(m.encoder.params.numel(), generator=g) * 2 - 1
        if family == 'half':
            u *= 0.5
        elif family == 'tiny':
            u *= 1e-4
        elif family == 'scaled':
            lvs = levels(m.grid)
            for lv in lvs:
                u[2 * lv['offset']:2 * (lv['offset'] + lv['entries'])] *= 0.5 * lvs[0]['scale'] / lv['scale']
        else:
            raise ValueError(family)
        m.encoder.params.copy_(u)


def network(kw, grid, family, scale, seed):
    from videoswap_amd.atlas import HashGridMLP
    torch.manual_seed(seed)
    m = HashGridMLP(**kw, grid=grid)                     # nn.Linear default initialisation
    with torch.no_grad():
        for lin in m.hidden:
            lin.weight.mul_(scale)
            lin.bias.mul_(scale)
    fill_table(m, family, seed)
    return m


def _weights(m, dtype):
    return ([lin.weight.detach().cpu().to(dtype) for lin in m.hidden], [lin.bias.detach().cpu().to(dtype) for lin in m.hidden])


def preactivations(m, x, dtype):
    """every hidden layer's pre-activation [N, (L - 1) * hidden] of the chain in `dtype`"""
    ws, bs = _weights(m, dtype)
    h = atlas_render_case.hash_encode(x, m.encoder.params, m.grid, dtype)
    inp, zs = h.clone(), []
    for i, (w, b) in enumerate(zip(ws[:-1], bs[:-1])):
        if i > 0:
            h = F.relu(h)
        if i in m.skip_layers:
            h = torch.cat((h, inp), 1)
        h = F.linear(h, w, b)
        zs.append(h)
    return torch.cat(zs, dim=1)


def candidates(N, seed, one_cell=None):
    """2 N + 64 rows uniform in [-1, 1)^2; one_cell = the finest scale: uniform inside one cell of that level"""
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(2 * N + 64, 2, generator=g)
    if one_cell is None:
        return u * 2 - 1
    # pos = scale x + 0.5 in [k + 0.05, k + 0.95): strictly inside the cell k, with room for the fp32 position's rounding
    k = torch.tensor([[round(0.3 * one_cell), round(-0.6 * one_cell)]], dtype=torch.float32)
    return (k + 0.05 + 0.9 * u - 0.5) / one_cell


def select_inputs(m, N, seed, one_cell=False):
    """-> (x [N, 2], share of the candidates dropped, delta)"""
    cand = candidates(N, seed, levels(m.grid)[-1]['scale'] if one_cell else None)
    with torch.no_grad():
        z64, z32 = preactivations(m, cand, torch.float64), preactivations(m, cand, torch.float32)
    delta = 16 * float((z32.double() - z64).abs().max())
    keep = ~(z64.abs() < delta).any(dim=1)
    dropped = 1.0 - float(keep.float().mean())
    assert dropped <= 0.5, (dropped, delta)
    x = cand[keep][:N]
    assert x.shape[0] == N
    return x.contiguous(), dropped, delta


def reference_grads(m, x, G, dtype):
    """[dW_0, db_0, dW_1, ..., d table, d x] of (y * G).sum() by autograd on the CPU in `dtype`"""
    ws, bs = _weights(m, dtype)
    params = [q.requires_grad_(True) for pair in zip(ws, bs) for q in pair]
    table = m.encoder.params.detach().cpu().to(dtype).requires_grad_(True)
    xd = x.detach().cpu().to(dtype).requires_grad_(True)
    y = hash_forward_diff(params[0::2], params[1::2], table, m.grid, xd, m.skip_layers, m.use_tanh)
    return list(torch.autograd.grad((y * G.to(dtype)).sum(), params + [table, xd]))


def module_grads(m, x):
    return [q.grad.detach().cpu() for lin in m.hidden for q in (lin.weight, lin.bias)] + [m.encoder.params.grad.detach().cpu(),
                                                                                          x.grad.detach().cpu()]


def backward_through(m, x, G):
    """one forward and one backward of the module on its own device, x requiring grad -> (y, the gradients), on the CPU"""
    dev = next(m.parameters()).device
    m.zero_grad()
    xg = x.detach().clone().to(dev).requires_grad_(True)
    y = m(xg)
    (y * G.to(dev)).sum().backward()
    return y.detach().cpu(), module_grads(m, xg)


def addressed(m, x):
    """bool [table floats]: the entries some corner of some row addresses"""
    hit = torch.zeros(m.encoder.params.numel() // 2, dtype=torch.bool)
    for _, _, idx in cells(x.cpu(), m.grid):
        for i in idx:
            hit[i] = True
    return hit.repeat_interleave(2)


# ------------------------------------------------------------------------------------------------
# CPU stand-ins of ops.hash_grid_backward / hash_mlp_train_workspace / hash_mlp_train_forward / hash_mlp_backward
# ------------------------------------------------------------------------------------------------
PLANTS = ('drop_corner', 'no_scale', 'flip_sign', 'skip_passes')


class HashFitStandin:
    """fp32 PyTorch on the CPU, the grid backward written out as include/vsx.h K17 states it (index_add for the table).
    `plant`: a wrong gradient for the tests of the rule's power: 'drop_corner' (corner 3 left out of the table gradient and
    of grad_x), 'no_scale' (the scale_l factor missing in grad_x), 'flip_sign' (corner 1's sign along x flipped),
    'skip_passes' (a skip layer's encoded columns pass their gradient on to the grid)."""

    def __init__(self, plant=None):
        assert plant is None or plant in PLANTS
        self.plant, self.forward_calls, self.backward_calls, self.grid_calls = plant, 0, 0, 0
        self.wanted = []

    def hash_grid_backward(self, x, grad_enc, table, grid, want_table=True, want_x=True):
        assert x.dtype == torch.float32 and x.dim() == 2 and x.shape[1] == 2 and x.is_contiguous() and table.dim() == 1
        assert grad_enc.shape == (x.shape[0], 2 * int(grid['n_levels'])) and grad_enc.dtype == torch.float32
        self.grid_calls += 1
        tab = table.detach().view(-1, 2)
        gt = torch.zeros_like(tab) if want_table else None
        gx = torch.zeros_like(x) if want_x else None
        for l, (lv, cell, idx) in enumerate(cells(x, grid)):
            scale = torch.tensor(lv['scale'], dtype=torch.float32)
            w = scale * x + 0.5 - cell
            ge = grad_enc[:, 2 * l:2 * l + 2]
            for c in range(4):
                if self.plant == 'drop_corner' and c == 3:
                    continue
                a0 = w[:, 0] if c & 1 else 1 - w[:, 0]
                a1 = w[:, 1] if c >> 1 else 1 - w[:, 1]
                if want_table:
                    gt.index_add_(0, idx[c], (a0 * a1).unsqueeze(1) * ge)
                if want_x:
                    t = (tab[idx[c]] * ge).sum(dim=1)
                    s = scale if self.plant != 'no_scale' else 1.0
                    sign0 = (1.0 if c & 1 else -1.0) * (-1.0 if self.plant == 'flip_sign' and c == 1 else 1.0)
                    gx[:, 0] += s * sign0 * a1 * t
                    gx[:, 1] += s * (1.0 if c >> 1 else -1.0) * a0 * t
        return (gt.reshape(-1) if want_table else None), gx

    @staticmethod
    def hash_mlp_train_workspace(N, grid, output_dim, hidden_dim, mlp_layers, skip_layers=(), input_dim=2):
        E, R = 2 * int(grid['n_levels']), 512
        grad = 0
        for l in range(mlp_layers):
            k = (hidden_dim if l > 0 else 0) + (E if l == 0 or l in skip_layers else 0)
            f = output_dim if l == mlp_layers - 1 else hidden_dim
            grad += f * k + f
        saved = N * ((mlp_layers - 1) * hidden_dim + E + output_dim)
        return saved, (N + R - 1) // R * grad + 2 * N * hidden_dim + N * output_dim + N * E, grad

    def hash_mlp_train_forward(self, x, table, grid, packed, output_dim, hidden_dim, mlp_layers, skip_layers=(), use_tanh=True,
                               saved=None):
        assert x.dtype == torch.float32 and x.dim() == 2 and x.is_contiguous() and saved is None
        assert not x.requires_grad and not table.requires_grad
        if x.shape[1] != 2:
            raise NotImplementedError(f'hash_mlp_train_forward: input_dim {x.shape[1]}')
        self.forward_calls += 1
        enc = atlas_render_case.hash_encode(x, table, grid, torch.float32)
        ws, bs = unpack(packed, enc.shape[1], output_dim, hidden_dim, mlp_layers, 'none', 0, list(skip_layers))
        h, acts = enc, []
        for i, (w, b) in enumerate(zip(ws, bs)):
            if i > 0:
                h = F.relu(h)
                acts.append(h)
            if i in skip_layers:
                h = torch.cat((h, enc), 1)
            h = F.linear(h, w, b)
        out = torch.tanh(h) if use_tanh else h
        return out, torch.cat([a.reshape(-1) for a in acts] + [enc.reshape(-1), out.reshape(-1)])

    def hash_mlp_backward(self, grad_out, x, table, grid, saved, packed, output_dim, hidden_dim, mlp_layers, skip_layers=(),
                          use_tanh=True, want_table=True, want_x=True, grad=None, scratch=None):
        assert grad_out.dtype == torch.float32 and grad_out.is_contiguous() and grad is None and scratch is None
        self.backward_calls += 1
        self.wanted.append((bool(want_table), bool(want_x)))
        N, L, E = grad_out.shape[0], mlp_layers, 2 * int(grid['n_levels'])
        ws, _ = unpack(packed, E, output_dim, hidden_dim, mlp_layers, 'none', 0, list(skip_layers))
        nh = (L - 1) * N * hidden_dim
        assert saved.numel() == nh + N * E + N * output_dim
        H = saved[:nh].view(L - 1, N, hidden_dim)
        enc, out = saved[nh:nh + N * E].view(N, E), saved[nh + N * E:].view(N, output_dim)
        dz = grad_out * (1 - out * out) if use_tanh else grad_out
        parts, denc = [None] * L, torch.zeros(N, E)
        for l in range(L - 1, -1, -1):
            inp = enc if l == 0 else (torch.cat((H[l - 1], enc), 1) if l in skip_layers else H[l - 1])
            parts[l] = torch.cat(((dz.t() @ inp).reshape(-1), dz.sum(dim=0)))
            if l == 0:
                denc = denc + dz @ ws[0]
            else:
                if self.plant == 'skip_passes' and l in skip_layers:
                    denc = denc + dz @ ws[l][:, hidden_dim:]
                dz = (dz @ ws[l][:, :hidden_dim]) * (H[l - 1] > 0)
        gt = gx = None
        if want_table or want_x:
            gt, gx = self.hash_grid_backward(x, denc.contiguous(), table, grid, want_table, want_x)
            self.grid_calls -= 1
        return torch.cat(parts), gt, gx


@contextlib.contextmanager
def hash_fit_standin(plant=None):
    """every atlas op on the CPU for the block: the coordinate and hash forwards, the K16 and the K17 training ops"""
    from atlas_fit_case import FitStandin
    s, h, c = HashFitStandin(plant), atlas_render_case.HashStandin(), FitStandin()
    with swapped(coord_mlp=atlas_case.Standin(), coord_mlp_train_forward=c.forward, coord_mlp_backward=c.backward,
                 hash_mlp=h.hash_mlp, hash_grid=h.hash_grid, hash_grid_backward=s.hash_grid_backward,
                 hash_mlp_train_workspace=s.hash_mlp_train_workspace, hash_mlp_train_forward=s.hash_mlp_train_forward,
                 hash_mlp_backward=s.hash_mlp_backward):
        yield s


# ------------------------------------------------------------------------------------------------
# atlas.fit_reconstruction on a toy atlas, and its fp64 restatement
# ------------------------------------------------------------------------------------------------
FIT = dict(res_x=48, res_y=32, frames=4, iters=20, batch=1024, lr=1e-4, seed=21)
FIT_NETWORKS = ('FG_UV_Mapping', 'BG_UV_Mapping', 'F_Alpha', 'F_Atlas')


def toy_atlas(seed=3):
    """(models on the CPU: hidden 64, SMALL_GRID; video [H, W, 3, T] in [0, 1]; masks [H, W, T] in {0, 1})"""
    models = atlas_render_case.toy_models(atlas_render_case.toy_config(hidden=64), grid=SMALL_GRID, seed=seed)
    W, H, T = FIT['res_x'], FIT['res_y'], FIT['frames']
    ys, xs, ts = torch.meshgrid(torch.arange(H) / H, torch.arange(W) / W, torch.arange(T) / T, indexing='ij')
    video = torch.stack((0.5 + 0.4 * torch.sin(6 * xs + ts), 0.5 + 0.4 * torch.cos(5 * ys - ts), 0.5 + 0.3 * torch.sin(4 * (xs + ys))), dim=2)
    masks = (((xs - 0.5 - 0.1 * ts) ** 2 + (ys - 0.5) ** 2) < 0.08).to(torch.float32)
    return models, video.contiguous(), masks.contiguous()


def run_fit(models, video, masks, device, **over):
    """atlas.fit_reconstruction on copies of `models` on `device`, the generator seeded -> (history, the trained copies)"""
    import copy
    from videoswap_amd import atlas
    cfg = dict(FIT, **over)
    nets = {k: copy.deepcopy(m).to(device) for k, m in models.items()}
    torch.manual_seed(cfg['seed'])
    history = atlas.fit_reconstruction(nets, video, masks, cfg['iters'], batch=cfg['batch'], lr=cfg['lr'],
                                       train=cfg.get('train', FIT_NETWORKS))
    return history, nets


def fit_fp64(models, video, masks):
    """the same steps restated in double precision on the CPU, on the same samples, all four networks trained -> the history"""
    W, H, T = FIT['res_x'], FIT['res_y'], FIT['frames']
    larger = max(W, H)
    par = {k: [q.requires_grad_(True) for pair in zip(*_weights(models[k], torch.float64)) for q in pair] for k in FIT_NETWORKS}
    atlas_net = models['F_Atlas']
    table = atlas_net.encoder.params.detach().double().requires_grad_(True)

    def coord(k, x):
        m = models[k]
        return mlp_forward(par[k][0::2], par[k][1::2], x, m.pe_type, m.pe_dim, m.skip_layers, m.use_tanh)

    # the parameters in the order fit_reconstruction hands them to Adam (one group: the order does not change a step)
    params = par['FG_UV_Mapping'] + par['BG_UV_Mapping'] + par['F_Alpha'] + [table] + par['F_Atlas']
    optimizer = torch.optim.Adam(params, lr=FIT['lr'])
    torch.manual_seed(FIT['seed'])
    history = []
    for _ in range(FIT['iters']):
        idx = torch.randint(T * H * W, (FIT['batch'], 1))
        f, rem = idx // (H * W), idx % (H * W)
        i, j = rem // W, rem % W
        rgb = video[i, j, :, f].squeeze(1).double()
        alpha_gt = masks[i, j, f].squeeze(1).double().unsqueeze(-1)
        xyt = torch.cat([j / (larger / 2) - 1, i / (larger / 2) - 1, f / (T / 2) - 1], dim=1).double()   # rounded to fp32 first
        uv_fg, uv_bg = coord('FG_UV_Mapping', xyt), coord('BG_UV_Mapping', xyt)
        alpha = 0.5 * (coord('F_Alpha', xyt) + 1.0)
        alpha = alpha * 0.99
        alpha = alpha + 0.001
        both = hash_forward_diff(par['F_Atlas'][0::2], par['F_Atlas'][1::2], table, atlas_net.grid,
                                 torch.cat((uv_fg * 0.5 + 0.5, uv_bg * 0.5 - 0.5), dim=0), atlas_net.skip_layers, atlas_net.use_tanh)
        n = xyt.shape[0]
        fg, bg = (both[:n] + 1.0) * 0.5, (both[n:] + 1.0) * 0.5
        out = fg * alpha + bg * (1.0 - alpha)
        loss = 5000.0 * (torch.norm(out - rgb, dim=1) ** 2).mean()
        loss = loss + 2000.0 * torch.mean(-alpha_gt * torch.log(alpha) - (1 - alpha_gt) * torch.log(1 - alpha))
        loss = loss + 1000.0 * (torch.norm(fg * (1.0 - alpha), dim=1) ** 2).mean()
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
        history.append(loss.item())
    return history


def history_diff(a, b):
    assert len(a) == len(b)
    return max(abs(x - y) for x, y in zip(a, b))
