"""Shared pieces of tests/test_atlas_fit.py (CPU) and tests/test_atlas_fit_gpu.py: the gradient cases, the fp64 reference,
the input selection, the comparison rule, the CPU stand-ins of the two training ops (pure PyTorch; they UNPACK the kernel's
weight buffer like atlas_case.unpack and keep `saved` in the layout of include/vsx.h K16), the pretrain_mapping fixture
rule and the fp64 restatement of the inverse-mapping fit.

Reference: autograd of the F.linear chain of atlas_case.mlp_forward on the CPU (the skip input is a copy of x, which has no
gradient), scalar (y * G).sum() for a fixed G ~ normal(0, 1) / N.

Input selection: a ReLU whose pre-activation lies within rounding of zero has a legitimately different mask in fp32 and in
fp64.  Such rows are removed from the INPUTS, from the references alone, before anything runs on the GPU: of 2 N + 64
candidates, uniform in [-1, 1), every row with a hidden pre-activation |z| < delta in fp64 is dropped, delta = 16 x the
largest fp32-vs-fp64 pre-activation difference; the first N survivors are used; at most half may be dropped (asserted).

Rule: per parameter tensor e = max |g - g64| / max |g64|; E = the largest e of a case; E_kernel <= 4 E_fp32torch on the
same inputs (the project's margin for another summation order, as in tests/test_atlas_gpu.py).
"""
import contextlib
import os

import torch
import torch.nn.functional as F

from atlas_case import mlp_forward, swapped, unpack
from util import GOLDEN

FIXTURE = os.path.join(GOLDEN, 'atlas_pretrain.pt')
R = 512                       # ops.COORD_MLP_WGRAD_ROWS (asserted in test_atlas_fit.py)

FG = dict(input_dim=3, output_dim=2, hidden_dim=256, pe_type='none', pe_dim=4, mlp_layers=6, skip_layers=[])
INV = dict(FG, output_dim=3)
BG = dict(FG, mlp_layers=4)
ALPHA = dict(input_dim=3, output_dim=1, hidden_dim=256, pe_type='encoding', pe_dim=5, mlp_layers=8, skip_layers=[])
SKIP = dict(input_dim=2, output_dim=3, hidden_dim=256, pe_type='encoding', pe_dim=4, mlp_layers=8, skip_layers=[4, 7])
CASES = [('fg', FG, n) for n in (1, 63, 64, 65, R + 1, 10000)] + [
    ('inverse', INV, 1000), ('bg', BG, 1000), ('alpha', ALPHA, 1000), ('skip_4_7', SKIP, 1000),
    ('hidden64', dict(FG, hidden_dim=64), 1000), ('hidden32', dict(ALPHA, hidden_dim=32), 1000),
    ('no_tanh', dict(INV, use_tanh=False, hidden_dim=128, mlp_layers=2), 65)]
# weights at the nn.Linear default initialisation and at twice that scale; the 10 000-row case runs once
RUNS = [c + (s,) for c in CASES for s in (1.0, 2.0) if not (c[2] >= 10000 and s != 1.0)]
RUN_IDS = [f'{c[0]}-{c[2]}-x{c[3]:g}' for c in RUNS]


def network(kw, scale, seed):
    from videoswap_amd.atlas import CoordMLP
    torch.manual_seed(seed)
    m = CoordMLP(**kw)                                   # nn.Linear default initialisation
    with torch.no_grad():
        for q in m.parameters():
            q.mul_(scale)
    return m


def _weights(m, dtype):
    return ([lin.weight.detach().cpu().to(dtype) for lin in m.hidden], [lin.bias.detach().cpu().to(dtype) for lin in m.hidden])


def preactivations(m, x, dtype):
    """every hidden layer's pre-activation [N, (L - 1) * hidden] of the F.linear chain in `dtype`"""
    ws, bs = _weights(m, dtype)
    x = x.to(dtype)
    if m.pe_type == 'encoding':
        from atlas_case import encode
        x = encode(x, m.pe_dim)
    inp, zs = x.clone(), []
    for i, (w, b) in enumerate(zip(ws[:-1], bs[:-1])):
        if i > 0:
            x = F.relu(x)
        if i in m.skip_layers:
            x = torch.cat((x, inp), 1)
        x = F.linear(x, w, b)
        zs.append(x)
    return torch.cat(zs, dim=1)


def select_inputs(m, N, seed):
    """-> (x [N, input_dim], share of the candidates dropped, delta)"""
    g = torch.Generator().manual_seed(seed)
    cand = torch.rand(2 * N + 64, m.input_dim, generator=g) * 2 - 1
    with torch.no_grad():
        z64, z32 = preactivations(m, cand, torch.float64), preactivations(m, cand, torch.float32)
    delta = 16 * float((z32.double() - z64).abs().max())
    keep = ~(z64.abs() < delta).any(dim=1)
    dropped = 1.0 - float(keep.float().mean())
    assert dropped <= 0.5, (dropped, delta)
    x = cand[keep][:N]
    assert x.shape[0] == N
    return x.contiguous(), dropped, delta


def cotangent(N, output_dim, seed):
    g = torch.Generator().manual_seed(seed + 77)
    return torch.randn(N, output_dim, generator=g) / N


def reference_grads(m, x, G, dtype):
    """[dW_0, db_0, dW_1, ...] of (y * G).sum() by autograd on the CPU in `dtype`"""
    ws, bs = _weights(m, dtype)
    params = [q.requires_grad_(True) for pair in zip(ws, bs) for q in pair]
    y = mlp_forward(params[0::2], params[1::2], x.to(dtype), m.pe_type, m.pe_dim, m.skip_layers, m.use_tanh)
    return list(torch.autograd.grad((y * G.to(dtype)).sum(), params))


def module_grads(m):
    return [q.grad.detach().cpu() for lin in m.hidden for q in (lin.weight, lin.bias)]


def worst_error(grads, grads64):
    """E of the rule: the largest max |g - g64| / max |g64| over the parameter tensors"""
    assert len(grads) == len(grads64)
    worst = 0.0
    for g, g64 in zip(grads, grads64):
        assert g.shape == g64.shape, (g.shape, g64.shape)
        worst = max(worst, float((g.double() - g64).abs().max() / g64.abs().max()))
    return worst


def backward_through(m, x, G):
    """one forward and one backward of the module on its own device -> (y on the CPU, the gradients on the CPU)"""
    dev = next(m.parameters()).device
    m.zero_grad()
    y = m(x.to(dev))
    (y * G.to(dev)).sum().backward()
    return y.detach().cpu(), module_grads(m)


# ------------------------------------------------------------------------------------------------
# CPU stand-ins of ops.coord_mlp_train_forward / ops.coord_mlp_backward
# ------------------------------------------------------------------------------------------------
class FitStandin:
    """fp32 PyTorch on the CPU; `plant`: a wrong gradient for the tests of the rule's power ('drop_row': one input row left
    out of every dW, 'wrong_mask': the ReLU mask of the layer below, 'no_tanh': the tanh factor omitted)"""

    def __init__(self, plant=None):
        self.plant, self.forward_calls, self.backward_calls = plant, 0, 0

    @staticmethod
    def _check(pe_type, mlp_type):
        if pe_type not in ('none', 'encoding'):
            raise NotImplementedError(f'coord_mlp: pe_type {pe_type!r}')
        if mlp_type != 'origin':
            raise NotImplementedError(f'coord_mlp: mlp_type {mlp_type!r}')

    def forward(self, x, packed, input_dim, output_dim, hidden_dim, mlp_layers, pe_type='none', pe_dim=0, mlp_type='origin',
                skip_layers=(), use_tanh=True, saved=None):
        self._check(pe_type, mlp_type)
        assert x.dtype == torch.float32 and x.dim() == 2 and x.shape[1] == input_dim and x.is_contiguous() and saved is None
        self.forward_calls += 1
        ws, bs = unpack(packed, input_dim, output_dim, hidden_dim, mlp_layers, pe_type, pe_dim, list(skip_layers))
        h = x
        if pe_type == 'encoding':
            from atlas_case import encode
            h = encode(x, pe_dim)
        enc, acts = h.clone(), []
        for i, (w, b) in enumerate(zip(ws, bs)):
            if i > 0:
                h = F.relu(h)
                acts.append(h)
            if i in skip_layers:
                h = torch.cat((h, enc), 1)
            h = F.linear(h, w, b)
        out = torch.tanh(h) if use_tanh else h
        return out, torch.cat([a.reshape(-1) for a in acts] + [enc.reshape(-1), out.reshape(-1)])

    def backward(self, grad_out, saved, packed, input_dim, output_dim, hidden_dim, mlp_layers, pe_type='none', pe_dim=0,
                 mlp_type='origin', skip_layers=(), use_tanh=True, grad=None):
        self._check(pe_type, mlp_type)
        assert grad_out.dtype == torch.float32 and grad_out.is_contiguous() and grad is None
        self.backward_calls += 1
        ws, _ = unpack(packed, input_dim, output_dim, hidden_dim, mlp_layers, pe_type, pe_dim, list(skip_layers))
        N, L, E = grad_out.shape[0], mlp_layers, 2 * input_dim * pe_dim if pe_type == 'encoding' else input_dim
        nh = (L - 1) * N * hidden_dim
        assert saved.numel() == nh + N * E + N * output_dim
        H = saved[:nh].view(L - 1, N, hidden_dim)
        enc, out = saved[nh:nh + N * E].view(N, E), saved[nh + N * E:].view(N, output_dim)
        dz = grad_out * (1 - out * out) if use_tanh and self.plant != 'no_tanh' else grad_out
        parts = [None] * L
        for l in range(L - 1, -1, -1):
            inp = enc if l == 0 else (torch.cat((H[l - 1], enc), 1) if l in skip_layers else H[l - 1])
            rows = dz
            if self.plant == 'drop_row' and N > 0:
                rows = dz.clone()
                rows[N // 2] = 0
            parts[l] = torch.cat(((rows.t() @ inp).reshape(-1), dz.sum(dim=0)))
            if l > 0:
                mask = H[l - 2 if self.plant == 'wrong_mask' and l >= 2 else l - 1] > 0
                dz = (dz @ ws[l][:, :hidden_dim]) * mask
        return torch.cat(parts)


@contextlib.contextmanager
def fit_standin(plant=None):
    """the three coordinate-MLP ops on the CPU for the block"""
    from atlas_case import Standin
    s = FitStandin(plant)
    with swapped(coord_mlp=Standin(), coord_mlp_train_forward=s.forward, coord_mlp_backward=s.backward):
        yield s


# ------------------------------------------------------------------------------------------------
# pretrain_mapping against the reference's own run (tests/golden/make_golden_atlas_fit.py)
# ------------------------------------------------------------------------------------------------
def check_pretrain_fixture(device):
    """Our pretrain_mapping from the recorded initial weights, with the reference's seed (so: its samples), against the
    reference's fp64 run: per seed the max-abs probe difference, and the difference of the returned loss, must be at most
    4 x the largest fp32-reference-vs-fp64 difference over the seeds.  Returns the figures."""
    from videoswap_amd import atlas
    fix = torch.load(FIXTURE, map_location='cpu', weights_only=True)
    runs = fix['runs']
    bound_probe = 4 * max(float((r['probe_fp32'].double() - r['probe_fp64']).abs().max()) for r in runs)
    bound_loss = 4 * max(abs(r['loss_fp32'] - r['loss_fp64']) for r in runs)
    figures = []
    for r in runs:
        torch.manual_seed(r['seed'])
        m = atlas.CoordMLP(**fix['spec'])                  # consumes the generator as IMLP_Hash's constructor did
        for k, v in m.state_dict().items():
            assert torch.equal(v, r['initial'][k]), k      # hence the same initial weights, and the same samples from here on
        m = m.to(device)
        m, loss = atlas.pretrain_mapping(m, fix['scale'], fix['res_x'], fix['res_y'], fix['frames'], pretrain_iters=fix['iters'])
        assert not m._differentiable                       # the switch is back where it was
        with torch.no_grad():
            y = m(fix['probe'].to(device)).cpu()
        figures.append(dict(seed=r['seed'], probe_diff=float((y.double() - r['probe_fp64']).abs().max()),
                            loss_diff=abs(loss - r['loss_fp64']), bound_probe=bound_probe, bound_loss=bound_loss))
    print('pretrain_mapping vs the fp64 reference:', figures)
    for f in figures:
        assert f['probe_diff'] <= bound_probe and f['loss_diff'] <= bound_loss, f
    return figures


# ------------------------------------------------------------------------------------------------
# the inverse-mapping fit: random hidden-64 networks and an fp64 restatement of train_atlas.py:255-266
# ------------------------------------------------------------------------------------------------
FIT = dict(res_x=96, res_y=64, frames=8, iters=30, batch=2048, seed=11)
FIT_SPECS = {'FG_UV_Mapping': dict(FG, hidden_dim=64), 'FG_UV_Mapping_Inverse': dict(INV, hidden_dim=64),
             'F_Alpha': dict(ALPHA, hidden_dim=64)}


def fit_networks(alpha_shift=None):
    """the three networks on the CPU, seeded; F_Alpha's last bias is moved by minus the median of its pre-tanh output
    over a probe, so that about half the rows are foreground (`alpha_shift` replaces that)"""
    nets = {k: network(kw, 2.0, seed=300 + i) for i, (k, kw) in enumerate(FIT_SPECS.items())}
    g = torch.Generator().manual_seed(5)
    probe = torch.rand(4096, 3, generator=g) * 2 - 1
    a = nets['F_Alpha']
    with torch.no_grad():
        z = torch.atanh(mlp_forward(*_weights(a, torch.float64), probe.double(), a.pe_type, a.pe_dim, a.skip_layers, True))
        a.hidden[-1].bias.sub_(float(z.median()) if alpha_shift is None else -alpha_shift)
    return nets


def run_fit(nets, device, **over):
    """atlas.fit_inverse_mapping on copies of `nets` on `device`, with the generator seeded"""
    import copy
    from videoswap_amd import atlas
    cfg = dict(FIT, **over)
    nets = {k: copy.deepcopy(m).to(device) for k, m in nets.items()}
    torch.manual_seed(cfg['seed'])
    return atlas.fit_inverse_mapping(nets['FG_UV_Mapping'], nets['FG_UV_Mapping_Inverse'], nets['F_Alpha'], cfg['res_x'],
                                     cfg['res_y'], cfg['frames'], iters=cfg['iters'], batch=cfg['batch'], holdout=512)


def fit_fp64(nets):
    """the same steps restated in double precision on the CPU, on the same samples -> the loss history"""
    W, H, T = FIT['res_x'], FIT['res_y'], FIT['frames']
    larger = max(W, H)
    par = {k: [q.requires_grad_(k == 'FG_UV_Mapping_Inverse') for pair in zip(*_weights(m, torch.float64)) for q in pair]
           for k, m in nets.items()}

    def run(k, x):
        m = nets[k]
        return mlp_forward(par[k][0::2], par[k][1::2], x, m.pe_type, m.pe_dim, m.skip_layers, m.use_tanh)

    optimizer = torch.optim.Adam(par['FG_UV_Mapping_Inverse'], lr=1e-4)
    torch.manual_seed(FIT['seed'])
    history = []
    for _ in range(FIT['iters']):
        idx = torch.randint(T * H * W, (FIT['batch'], 1))
        f, rem = idx // (H * W), idx % (H * W)
        xyt = torch.cat([(rem % W) / (larger / 2) - 1, (rem // W) / (larger / 2) - 1, f / (T / 2) - 1], dim=1).double()
        with torch.no_grad():
            xyt = xyt[(0.5 * (run('F_Alpha', xyt) + 1.0) > 0.5).squeeze(1)]
            uv = run('FG_UV_Mapping', xyt)
        pred = run('FG_UV_Mapping_Inverse', torch.cat([uv, xyt[:, -1:]], dim=-1))
        loss = (pred - xyt).norm(dim=1).mean()
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
        history.append(loss.item())
    return history


def history_diff(a, b):
    assert len(a) == len(b)
    return max(abs(x - y) for x, y in zip(a, b))
