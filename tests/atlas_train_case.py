"""Shared pieces of tests/test_atlas_train.py (CPU), tests/test_atlas_train_gpu.py and tests/golden/make_golden_atlas_train.py:

* a dtype-generic torch restatement of one step of train_atlas.py:135-249 with the loss definitions of
  videoswap/atlas/loss_utils.py (`step_restated`).  It asks an EVALUATOR for every network output, block by block, in the
  reference's own order (each mapping network up to seven calls, the flow matches compacted with torch.where), so one
  loss code serves real networks (`NetEval`: the reference's separate calls), tiny closed-form callables (the golden) and
  prescribed network outputs (`TableEval`: K18b alone).  The pixel data come from a `Queries` object built the
  reference's way from (jif, data_dict) or from the outputs of the batch gather;
* `batch_restated`: K18a as torch statements on the CPU, the reference's own expressions (int64 / python float -> fp32);
* `TrainStandin`: CPU stand-ins of ops.atlas_batch / ops.atlas_losses (fp32 autograd of the restatement), with planted
  errors for the tests of the rule's power;
* `synthetic_data`: a data_dict with smooth frames, translation flows with sub-pixel parts and random 0/1 flow masks;
* the input families, the kink exclusion and the rules of the K18b parity tests.

Rules.  Gradients: per tensor e = max |g - g64| / max |g64|, E = the largest e of a case, E_kernel <= 4 E_fp32torch on the
same inputs (the project's margin for another summation order).  Loss values: |L - L64| <= max(4 |L32 - L64|, c 2^-24 A),
A = the fp64 mean of the absolute per-row terms; every per-row term of every loss is non-negative (squares, norms, |x|, a
cross-entropy), so A is the fp64 value itself, and c = `value_ops(N)`.
"""
import contextlib

import torch

from atlas_case import swapped

LOSS_CFG = {'reconstruction_loss': {'rgb_loss_weight': 5000.0, 'gradient_loss_weight': 1000.0, 'alpha_loss_weight': 2000.0},
            'rigidity_loss': {'rigidity_loss_weight': 1.0, 'global_rigidity_fg_loss_weight': 5.0, 'global_rigidity_bg_loss_weight': 50.0},
            'flow_loss': {'flow_loss_weight': 5.0, 'alpha_flow_loss_weight': 49.0},
            'sparsity_loss': {'sparsity_loss_weight': 1000.0}}
# train: of the reference's atlas YAMLs, but for the two iteration counts
TRAIN = dict(uv_mapping_scale=0.8, derivative_amount=1, global_derivative_amount=100, pretrain_alpha_iter=50000,
             pretrain_global_rigidity_iter=5000, loss_cfg=LOSS_CFG, optimizer={'type': 'Adam', 'lr': 1e-4})
LOSSES = ('gradient_loss', 'rgb_loss', 'alpha_loss', 'sparsity_loss', 'rigidity_loss_fg', 'rigidity_loss_bg', 'global_rigidity_loss_fg',
          'global_rigidity_loss_bg', 'flow_loss_fg', 'flow_loss_bg', 'flow_alpha_loss', 'total_loss', 'alpha_mean_fg', 'alpha_mean_bg')
NS = (0, 1, 63, 64, 65, 255, 256, 257, 513)
PLANTS = ('flow_alpha_path', 'gradient_block0', 'no_larger_dim', 'swap_jacobian', 'mean_over_N')
# the order in which one step of the reference calls each network: (block, layer) per call
CALL_ORDER = {'FG_UV_Mapping': [0, 2, 1, (3, 4), (5, 6), 7, 8], 'BG_UV_Mapping': [0, 2, 1, (3, 4), (5, 6), 7, 8],
              'F_Alpha': [0, 1, 2, 7, 8], 'F_Atlas': [(0, 'fg'), (0, 'bg'), (2, 'fg'), (1, 'fg'), (2, 'bg'), (1, 'bg')]}


def value_ops(N):
    """c of the value rule, counted from csrc/atlas_loss.hip in roundings of relative size 2^-24: the longest per-row chain
    is the rigidity term: a Jacobian entry 4 (difference, * larger_dim, / scale, / d); an entry of JtJ 2 x 4 + 1 + 1 = 10; the
    determinant 2 x 11 + 1 + 1 = 24; an entry of the inverse 11 + 24 + 1 = 36; its square 73, the two sums 75, the square root
    halves it and adds one: 39; l1 + l2: 40.  Then the reduction: 6 shuffle levels, 3 adds over the waves, one add per further
    workgroup, the division: 10 + (ceil(N / 256) - 1).  total_loss adds a product and an add per term: 11 more (used for
    every entry: the largest count)."""
    return 40 + 10 + max(0, (N + 255) // 256 - 1) + 11


def norm_funcs(larger_dim, T):
    return (lambda x: x / (larger_dim / 2) - 1), (lambda x: x / (T / 2) - 1)


def jif_of(idx, H, W):
    """flat indices [N, 1] in get_tuples' (frame, row, column) order -> jif [3, N, 1] = (column, row, frame)"""
    idx = idx.reshape(-1, 1)
    rem = idx % (H * W)
    return torch.stack((rem % W, rem // W, idx // (H * W)))


def squash(a):
    a = 0.5 * (a + 1.0)
    a = a * 0.99
    return a + 0.001


# ------------------------------------------------------------------------------------------------
# where a step's pixel data and query rows come from
# ------------------------------------------------------------------------------------------------
class Queries:
    """rows(block) -> the fp32 query rows of a block (a pair of blocks: both, stacked; 7 / 8: the relevant rows only);
    rgb, rgb_dx, rgb_dy [N, 3], alpha_gt [N, 1] (fp32); rel_f, rel_b: the batch indices of the relevant flow rows"""

    @classmethod
    def from_data(cls, jif, data, d, D):
        """the reference's way: fancy indexing of the data_dict and torch.where on the flow masks"""
        q = cls()
        H, W, _, T = data['video_frames'].shape
        q.larger, q.N = max(H, W), jif.shape[1]
        ns, nt = norm_funcs(q.larger, T)
        j, i, f = jif[0], jif[1], jif[2]
        jj, ii, ff = j.squeeze(1), i.squeeze(1), f.squeeze(1)
        q.rgb, q.rgb_dx, q.rgb_dy = (data[k][ii, jj, :, ff] for k in ('video_frames', 'video_frames_dx', 'video_frames_dy'))
        q.alpha_gt = data['mask_frames'][ii, jj, ff].unsqueeze(-1)
        t = nt(f)
        q._rows = {0: torch.cat([ns(j), ns(i), t], dim=1), 1: torch.cat([ns(j + 1), ns(i), t], dim=1),
                   2: torch.cat([ns(j), ns(i + 1), t], dim=1)}
        for blocks, amount in (((3, 4), d), ((5, 6), D)):
            q._rows[blocks] = torch.cat((ns(torch.cat([j, j - amount])), ns(torch.cat([i - amount, i])), nt(torch.cat([f, f]))), dim=1)
        for block, flows, mask, step in ((7, 'optical_flows', 'optical_flows_mask', 1), (8, 'optical_flows_reverse', 'optical_flows_reverse_mask', -1)):
            rel, level = torch.where(data[mask][ii, jj, ff, :])
            jr, ir, fr = jj[rel], ii[rel], ff[rel]
            fl = data[flows][ir, jr, :, fr, level]
            match = torch.stack((jr + fl[:, 0], ir + fl[:, 1], fr + step * 2 ** level))
            q._rows[block] = torch.stack([ns(match[0]), ns(match[1]), nt(match[2])]).T
            setattr(q, 'rel_f' if block == 7 else 'rel_b', rel)
        return q

    @classmethod
    def from_batch(cls, batch):
        """from the outputs of the batch gather (ops.atlas_batch's dict, on the CPU)"""
        q = cls()
        rows, B = batch['rows'], batch['rows'].shape[0]
        q.larger, q.N = batch['larger_dim'], rows.shape[1]
        q.rgb, q.rgb_dx, q.rgb_dy, q.alpha_gt = batch['rgb'], batch['rgb_dx'], batch['rgb_dy'], batch['alpha_gt'].unsqueeze(-1)
        q.rel_f, q.rel_b = torch.where(batch['m_fwd'])[0], torch.where(batch['m_bwd'])[0]
        q._rows = {0: rows[0], 1: rows[1], 2: rows[2], (3, 4): torch.cat((rows[3], rows[4])), 7: rows[B - 2][q.rel_f], 8: rows[B - 1][q.rel_b]}
        if B == 9:
            q._rows[(5, 6)] = torch.cat((rows[5], rows[6]))
        return q

    def rows(self, block):
        return self._rows[block]

    def to(self, device):
        """everything on `device` (the reference gathers on the CPU and moves each piece)"""
        for k in ('rgb', 'rgb_dx', 'rgb_dy', 'alpha_gt', 'rel_f', 'rel_b'):
            setattr(self, k, getattr(self, k).to(device))
        self._rows = {k: v.to(device) for k, v in self._rows.items()}
        return self


def batch_restated(idx, data, d, D, with_global=True):
    """K18a in torch on the CPU: every float by the reference's own expression -> the dict of ops.atlas_batch"""
    H, W, _, T = data['video_frames'].shape
    if data['optical_flows'].shape[-1] != 1:
        raise NotImplementedError(f"atlas_batch: {data['optical_flows'].shape[-1]} flow levels")
    ns, nt = norm_funcs(max(H, W), T)
    jif = jif_of(idx, H, W)
    j, i, f = jif[0], jif[1], jif[2]
    jj, ii, ff = j.squeeze(1), i.squeeze(1), f.squeeze(1)
    t = nt(f)
    blocks = [torch.cat([ns(j), ns(i), t], dim=1), torch.cat([ns(j + 1), ns(i), t], dim=1), torch.cat([ns(j), ns(i + 1), t], dim=1),
              torch.cat([ns(j), ns(i - d), t], dim=1), torch.cat([ns(j - d), ns(i), t], dim=1)]
    if with_global:
        blocks += [torch.cat([ns(j), ns(i - D), t], dim=1), torch.cat([ns(j - D), ns(i), t], dim=1)]
    for flows, step in (('optical_flows', 1), ('optical_flows_reverse', -1)):
        fl = data[flows][ii, jj, :, ff, 0]
        blocks.append(torch.stack([ns(jj + fl[:, 0]), ns(ii + fl[:, 1]), nt(ff + step)], dim=1))
    m_fwd = (data['optical_flows_mask'][ii, jj, ff, 0] != 0).to(torch.float32)
    m_bwd = (data['optical_flows_reverse_mask'][ii, jj, ff, 0] != 0).to(torch.float32)
    return dict(rows=torch.stack(blocks).to(torch.float32), rgb=data['video_frames'][ii, jj, :, ff], rgb_dx=data['video_frames_dx'][ii, jj, :, ff],
                rgb_dy=data['video_frames_dy'][ii, jj, :, ff], alpha_gt=data['mask_frames'][ii, jj, ff], m_fwd=m_fwd, m_bwd=m_bwd,
                counts=torch.tensor([int(m_fwd.sum()), int(m_bwd.sum())], dtype=torch.int32), larger_dim=max(H, W),
                with_global_rigidity=bool(with_global))


# ------------------------------------------------------------------------------------------------
# evaluators
# ------------------------------------------------------------------------------------------------
class NetEval:
    """the reference's separate calls: nets[name](x) per block, in `dtype`; every call is recorded (and keeps its gradient)"""

    def __init__(self, nets, dtype):
        self.nets, self.dtype, self.calls = nets, dtype, []

    def __call__(self, name, x, block, sel=None, layer=None):
        y = self.nets[name](x.to(self.dtype))
        if y.requires_grad:
            y.retain_grad()
        self.calls.append((name, block if layer is None else (block, layer), y))
        return y

    def outputs(self, name):
        return [y for n, _, y in self.calls if n == name]


class TableEval:
    """prescribed network outputs: uv_fg, uv_bg [B, N, 2], alpha_raw [5, N, 1], rgb_atlas [2, 3, N, 3] (layer, block)"""

    def __init__(self, uv_fg, uv_bg, alpha_raw, rgb_atlas):
        self.t = {'FG_UV_Mapping': uv_fg, 'BG_UV_Mapping': uv_bg, 'F_Alpha': alpha_raw, 'F_Atlas': rgb_atlas}
        self.B = uv_fg.shape[0]

    def _pos(self, name, block):
        if name == 'F_Alpha':
            return {0: 0, 1: 1, 2: 2, 7: 3, 8: 4}[block]
        return block if block < 5 or self.B == 9 else block - 2

    def __call__(self, name, x, block, sel=None, layer=None):
        if name == 'F_Atlas':
            return self.t[name][0 if layer == 'fg' else 1][block]
        if isinstance(block, tuple):
            return torch.cat([self.t[name][self._pos(name, b)] for b in block])
        y = self.t[name][self._pos(name, block)]
        return y if sel is None else y[sel]


# ------------------------------------------------------------------------------------------------
# the step
# ------------------------------------------------------------------------------------------------
def _mean0(x):
    """the mean; over no row 0 with a zero gradient (the project's convention; NaN in the reference)"""
    return x.mean() if x.numel() else x.sum()


def step_restated(ev, q, train, with_alpha, with_global, dtype, plant=None):
    """train_atlas.py:147-249 -> (loss_total, loss_dict); `train`: the YAML's train section"""
    assert plant is None or plant in PLANTS
    cfg, scale, larger = train['loss_cfg'], train['uv_mapping_scale'], q.larger
    rgb, rgb_dx, rgb_dy, alpha_gt = (v.to(dtype) for v in (q.rgb, q.rgb_dx, q.rgb_dy, q.alpha_gt))
    uv_fg, uv_bg = ev('FG_UV_Mapping', q.rows(0), 0), ev('BG_UV_Mapping', q.rows(0), 0)
    alpha = squash(ev('F_Alpha', q.rows(0), 0))
    rgb_fg = (ev('F_Atlas', uv_fg * 0.5 + 0.5, 0, layer='fg') + 1.0) * 0.5
    rgb_bg = (ev('F_Atlas', uv_bg * 0.5 - 0.5, 0, layer='bg') + 1.0) * 0.5
    rgb_out = rgb_fg * alpha + rgb_bg * (1.0 - alpha)
    loss_dict = {}

    # get_gradient_loss
    a_x1, a_y1 = squash(ev('F_Alpha', q.rows(1), 1)), squash(ev('F_Alpha', q.rows(2), 2))
    uvb_y1, uvb_x1 = ev('BG_UV_Mapping', q.rows(2), 2), ev('BG_UV_Mapping', q.rows(1), 1)
    uvf_y1, uvf_x1 = ev('FG_UV_Mapping', q.rows(2), 2), ev('FG_UV_Mapping', q.rows(1), 1)
    c1_y1 = (ev('F_Atlas', uvf_y1 * 0.5 + 0.5, 2, layer='fg') + 1.0) * 0.5
    c1_x1 = (ev('F_Atlas', uvf_x1 * 0.5 + 0.5, 1, layer='fg') + 1.0) * 0.5
    c2_y1 = (ev('F_Atlas', uvb_y1 * 0.5 - 0.5, 2, layer='bg') + 1.0) * 0.5
    c2_x1 = (ev('F_Atlas', uvb_x1 * 0.5 - 0.5, 1, layer='bg') + 1.0) * 0.5
    out_y1 = c1_y1 * a_y1 + c2_y1 * (1.0 - a_y1)
    out_x1 = c1_x1 * a_x1 + c2_x1 * (1.0 - a_x1)
    base = rgb_out.detach() if plant == 'gradient_block0' else rgb_out
    gradient_loss = torch.mean((rgb_dx - (out_x1 - base)).norm(dim=1) ** 2 + (rgb_dy - (out_y1 - base)).norm(dim=1) ** 2)
    loss_dict['gradient_loss'] = gradient_loss
    total = 0.0
    total += cfg['reconstruction_loss']['gradient_loss_weight'] * gradient_loss

    rgb_loss = (torch.norm(rgb_out - rgb, dim=1) ** 2).mean()
    loss_dict['rgb_loss'] = rgb_loss
    total += cfg['reconstruction_loss']['rgb_loss_weight'] * rgb_loss
    if with_alpha:
        alpha_loss = torch.mean(-alpha_gt * torch.log(alpha) - (1 - alpha_gt) * torch.log(1 - alpha))
        loss_dict['alpha_loss'] = alpha_loss
        total += cfg['reconstruction_loss']['alpha_loss_weight'] * alpha_loss
    loss_dict['alpha_mean_fg'] = alpha[alpha > 0.5].mean()
    loss_dict['alpha_mean_bg'] = alpha[alpha < 0.5].mean()
    sparsity = (torch.norm(rgb_fg * (1.0 - alpha), dim=1) ** 2).mean()
    loss_dict['sparsity_loss'] = sparsity
    total += cfg['sparsity_loss']['sparsity_loss_weight'] * sparsity

    def rigidity(name, uv0, amount, blocks):
        uv_p = ev(name, q.rows(blocks), blocks)                       # (x, y - amount, t) rows, then (x - amount, y, t) rows
        u_p, v_p = uv_p[:, 0].view(2, -1), uv_p[:, 1].view(2, -1)
        du, dv = uv0[:, 0].unsqueeze(0) - u_p, uv0[:, 1].unsqueeze(0) - v_p
        if plant == 'no_larger_dim':
            du_dx, du_dy, dv_dy, dv_dx = du[1], du[0], dv[0], dv[1]
        else:
            du_dx, du_dy, dv_dy, dv_dx = du[1] * larger / 2, du[0] * larger / 2, dv[0] * larger / 2, dv[1] * larger / 2
        if plant == 'swap_jacobian':
            du_dy, dv_dx = dv_dx, du_dy
        jac = torch.stack((torch.stack((du_dx, du_dy), dim=1), torch.stack((dv_dx, dv_dy), dim=1)), dim=1)
        jac = jac / scale
        jac = jac / amount
        jtj = torch.matmul(jac.transpose(1, 2), jac)
        a, b, c, e = jtj[:, 0, 0] + 0.001, jtj[:, 0, 1], jtj[:, 1, 0], jtj[:, 1, 1] + 0.001
        inv = torch.stack((torch.stack((e, -b), dim=1), torch.stack((-c, a), dim=1)), dim=1)
        inv = inv / (a * e - b * c).unsqueeze(-1).unsqueeze(-1)
        return ((jtj ** 2).sum(1).sum(1).sqrt() + (inv ** 2).sum(1).sum(1).sqrt()).mean()

    w = cfg['rigidity_loss']
    loss_dict['rigidity_loss_fg'] = rigidity('FG_UV_Mapping', uv_fg, train['derivative_amount'], (3, 4))
    total += w['rigidity_loss_weight'] * loss_dict['rigidity_loss_fg']
    loss_dict['rigidity_loss_bg'] = rigidity('BG_UV_Mapping', uv_bg, train['derivative_amount'], (3, 4))
    total += w['rigidity_loss_weight'] * loss_dict['rigidity_loss_bg']
    if with_global:
        loss_dict['global_rigidity_loss_fg'] = rigidity('FG_UV_Mapping', uv_fg, train['global_derivative_amount'], (5, 6))
        total += w['global_rigidity_fg_loss_weight'] * loss_dict['global_rigidity_loss_fg']
        loss_dict['global_rigidity_loss_bg'] = rigidity('BG_UV_Mapping', uv_bg, train['global_derivative_amount'], (5, 6))
        total += w['global_rigidity_bg_loss_weight'] * loss_dict['global_rigidity_loss_bg']

    def flow_mean(x):
        return x.sum() / q.N if plant == 'mean_over_N' else _mean0(x)

    def flow(name, uv0, weight):
        if plant == 'flow_alpha_path':
            weight = weight.detach()
        nxt = (ev(name, q.rows(7), 7, sel=q.rel_f) - uv0[q.rel_f]).norm(dim=1) * larger / (2 * scale)
        prv = (ev(name, q.rows(8), 8, sel=q.rel_b) - uv0[q.rel_b]).norm(dim=1) * larger / (2 * scale)
        return flow_mean(prv * weight[q.rel_b].squeeze(1)) * 0.5 + flow_mean(nxt * weight[q.rel_f].squeeze(1)) * 0.5

    w = cfg['flow_loss']
    loss_dict['flow_loss_fg'] = flow('FG_UV_Mapping', uv_fg, alpha)
    total += w['flow_loss_weight'] * loss_dict['flow_loss_fg']
    loss_dict['flow_loss_bg'] = flow('BG_UV_Mapping', uv_bg, 1 - alpha)
    total += w['flow_loss_weight'] * loss_dict['flow_loss_bg']
    a_next = squash(ev('F_Alpha', q.rows(7), 7, sel=q.rel_f))
    l_next = flow_mean((alpha[q.rel_f] - a_next).abs())
    a_prev = squash(ev('F_Alpha', q.rows(8), 8, sel=q.rel_b))
    l_prev = flow_mean((a_prev - alpha[q.rel_b]).abs())
    loss_dict['flow_alpha_loss'] = (l_next + l_prev) * 0.5
    total += w['alpha_flow_loss_weight'] * loss_dict['flow_alpha_loss']
    loss_dict['total_loss'] = total
    return total, loss_dict


def losses_vector(loss_dict, dtype):
    """[14] in the order LOSSES; a term that was not computed is 0"""
    return torch.stack([loss_dict[k].detach().to(dtype) if k in loss_dict else torch.zeros((), dtype=dtype) for k in LOSSES])


def train_of(cfg):
    """the flat cfg of ops.atlas_losses -> (train section, with_alpha)"""
    loss_cfg = {'reconstruction_loss': {k: cfg[k] for k in ('rgb_loss_weight', 'gradient_loss_weight', 'alpha_loss_weight')},
                'rigidity_loss': {k: cfg[k] for k in ('rigidity_loss_weight', 'global_rigidity_fg_loss_weight', 'global_rigidity_bg_loss_weight')},
                'flow_loss': {k: cfg[k] for k in ('flow_loss_weight', 'alpha_flow_loss_weight')},
                'sparsity_loss': {'sparsity_loss_weight': cfg['sparsity_loss_weight']}}
    return dict(uv_mapping_scale=cfg['uv_mapping_scale'], derivative_amount=cfg['derivative_amount'],
                global_derivative_amount=cfg['global_derivative_amount'], loss_cfg=loss_cfg), bool(cfg['with_alpha_loss'])


def flat_cfg(train=TRAIN, with_alpha=True):
    """the YAML's train section -> the flat cfg of ops.atlas_losses"""
    out = {k: v for group in train['loss_cfg'].values() for k, v in group.items()}
    out.update(uv_mapping_scale=train['uv_mapping_scale'], derivative_amount=train['derivative_amount'],
               global_derivative_amount=train['global_derivative_amount'], with_alpha_loss=bool(with_alpha))
    return out


def losses_from_outputs(uv_fg, uv_bg, alpha_raw, rgb_atlas, batch, cfg, dtype, plant=None):
    """the restatement on prescribed network outputs (flat, in the layouts of ops.atlas_losses) by autograd in `dtype` ->
    (losses [14], g_uv_fg, g_uv_bg, g_alpha_raw, g_rgb_atlas)"""
    B, N = batch['rows'].shape[0], batch['rows'].shape[1]
    train, with_alpha = train_of(cfg)
    with torch.enable_grad():                              # the stand-in runs inside an autograd Function's forward
        leaves = [t.detach().cpu().to(dtype).requires_grad_(True) for t in (uv_fg, uv_bg, alpha_raw, rgb_atlas)]
        ev = TableEval(leaves[0].view(B, N, 2), leaves[1].view(B, N, 2), leaves[2].view(5, N, 1), leaves[3].view(2, 3, N, 3))
        total, loss_dict = step_restated(ev, Queries.from_batch({k: (v.cpu() if torch.is_tensor(v) else v) for k, v in batch.items()}), train,
                                         with_alpha, B == 9, dtype, plant)
        grads = torch.autograd.grad(total, leaves, allow_unused=True)
    grads = [torch.zeros_like(t) if g is None else g for g, t in zip(grads, leaves)]
    return (losses_vector(loss_dict, dtype), *grads)


# ------------------------------------------------------------------------------------------------
# CPU stand-ins of ops.atlas_batch / ops.atlas_losses
# ------------------------------------------------------------------------------------------------
class TrainStandin:
    """fp32 PyTorch on the CPU; `plant`: a wrong loss path for the tests of the rule's power: 'flow_alpha_path' (alpha
    detached in the flow losses), 'gradient_block0' (rgb_output of block 0 detached in the gradient loss), 'no_larger_dim'
    (larger_dim / 2 missing in the Jacobian), 'swap_jacobian' (du_dy and dv_dx swapped), 'mean_over_N' (the flow means
    divide by N, not by the count of relevant rows)"""

    def __init__(self, plant=None):
        assert plant is None or plant in PLANTS
        self.plant, self.batch_calls, self.loss_calls = plant, 0, 0

    def atlas_batch(self, idx, data, derivative_amount, global_derivative_amount, with_global_rigidity=True):
        self.batch_calls += 1
        H, W, _, T = data['video_frames'].shape
        idx = idx.reshape(-1).cpu()
        assert idx.dtype == torch.int64
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= T * H * W):
            from videoswap_amd._lib import VsxError
            raise VsxError(f'atlas_batch: idx outside 0 .. {T * H * W - 1}')
        return batch_restated(idx, data, int(derivative_amount), int(global_derivative_amount), with_global_rigidity)

    def atlas_losses(self, uv_fg, uv_bg, alpha_raw, rgb_atlas, batch, cfg):
        self.loss_calls += 1
        N, B = batch['rgb'].shape[0], batch['rows'].shape[0]
        assert uv_fg.shape == (B * N, 2) and uv_bg.shape == (B * N, 2) and alpha_raw.numel() == 5 * N and rgb_atlas.shape == (6 * N, 3)
        assert all(t.dtype == torch.float32 and t.is_contiguous() for t in (uv_fg, uv_bg, alpha_raw, rgb_atlas))
        return losses_from_outputs(uv_fg, uv_bg, alpha_raw, rgb_atlas, batch, cfg, torch.float32, self.plant)


@contextlib.contextmanager
def train_standin(plant=None):
    """every atlas op on the CPU for the block: the network ops of hash_fit_case.hash_fit_standin and the two of K18"""
    from hash_fit_case import hash_fit_standin
    s = TrainStandin(plant)
    with hash_fit_standin(), swapped(atlas_batch=s.atlas_batch, atlas_losses=s.atlas_losses):
        yield s


# ------------------------------------------------------------------------------------------------
# synthetic data and network outputs
# ------------------------------------------------------------------------------------------------
def synthetic_data(W, H, T, seed=0):
    """a data_dict in load_input_data's layouts (fp32, CPU): smooth frames and their forward differences, a moving disc as
    the mask, translation flows with sub-pixel parts (0 on the frame that has no neighbour), random 0/1 flow masks"""
    g = torch.Generator().manual_seed(seed)
    ys, xs, ts = torch.meshgrid(torch.arange(H) / H, torch.arange(W) / W, torch.arange(T) / T, indexing='ij')
    video = torch.stack((0.5 + 0.4 * torch.sin(6 * xs + ts), 0.5 + 0.4 * torch.cos(5 * ys - ts), 0.5 + 0.3 * torch.sin(4 * (xs + ys))), dim=2)
    dx, dy = torch.zeros_like(video), torch.zeros_like(video)
    dy[:-1] = video[1:] - video[:-1]
    dx[:, :-1] = video[:, 1:] - video[:, :-1]
    masks = (((xs - 0.5 - 0.1 * ts) ** 2 + (ys - 0.5) ** 2) < 0.08).to(torch.float32)
    flows, flows_rev = torch.zeros(H, W, 2, T, 1), torch.zeros(H, W, 2, T, 1)
    fmask, rmask = torch.zeros(H, W, T, 1), torch.zeros(H, W, T, 1)
    for f in range(T - 1):
        shift = torch.rand(2, generator=g) * 3 - 1.5                      # a translation with a sub-pixel part
        wobble = 0.25 * torch.stack((torch.sin(7 * ys[:, :, 0]), torch.cos(5 * xs[:, :, 0])), dim=2)
        flows[:, :, :, f, 0] = shift + wobble
        flows_rev[:, :, :, f + 1, 0] = -shift - wobble
        fmask[:, :, f, 0] = (torch.rand(H, W, generator=g) < 0.6).to(torch.float32)
        rmask[:, :, f + 1, 0] = (torch.rand(H, W, generator=g) < 0.6).to(torch.float32)
    return {'video_frames': video.contiguous(), 'video_frames_dx': dx, 'video_frames_dy': dy, 'mask_frames': masks.contiguous(),
            'optical_flows': flows, 'optical_flows_reverse': flows_rev, 'optical_flows_mask': fmask, 'optical_flows_reverse_mask': rmask}


def sample(data, N, seed, corners=False):
    """N flat indices (int64 [N, 1]); corners: the first rows are the four image corners on frame 0 and on frame T - 1"""
    H, W, _, T = data['video_frames'].shape
    idx = torch.randint(T * H * W, (N, 1), generator=torch.Generator().manual_seed(seed + 5))
    if corners:
        c = [f * H * W + i * W + j for f in (0, T - 1) for i in (0, H - 1) for j in (0, W - 1)]
        idx[:min(N, 8), 0] = torch.tensor(c[:N], dtype=torch.int64)
    return idx


def with_masks(batch, mode):
    """a copy of a batch with prescribed flow relevance: 'none', 'one' (the middle row) or 'all'; 'data': unchanged"""
    out = dict(batch)
    if mode == 'data':
        return out
    N = batch['rgb'].shape[0]
    m = torch.zeros(N) if mode != 'all' else torch.ones(N)
    if mode == 'one' and N:
        m[N // 2] = 1.0
    out['m_fwd'], out['m_bwd'] = m.clone(), m.clone()
    out['counts'] = torch.tensor([int(m.sum()), int(m.sum())], dtype=torch.int32)
    return out


KINK = 1e-4
KINK_CAP = 0.05


def synthetic_outputs(N, batch, train, seed):
    """network outputs of the K18b tests, flat fp32: uv uniform in [-1, 1); the offset blocks uv minus a step that makes the
    Jacobians identity + 0.3 normal; the flow matches uv plus an error of about a pixel; alpha_raw uniform in (-0.999,
    0.999); rgb_atlas uniform in [-1, 1).  Rows within KINK of a kink (|alpha - alpha_match|, |alpha - 0.5|, a flow error
    norm; judged on these fp32 values as fp64, before anything runs) are replaced by the next candidates; at most KINK_CAP
    of the candidates may go -> (uv_fg, uv_bg, alpha_raw, rgb_atlas, the dropped share)"""
    g = torch.Generator().manual_seed(seed)
    B, larger, scale = batch['rows'].shape[0], batch['larger_dim'], train['uv_mapping_scale']
    M = N + N // 8 + 8
    pixel = 2 * scale / larger                                               # one pixel in uv units

    def mapping():
        uv = torch.rand(M, 2, generator=g) * 2 - 1
        blocks = [uv, uv + pixel * torch.randn(M, 2, generator=g), uv + pixel * torch.randn(M, 2, generator=g)]
        for amount in (train['derivative_amount'], train['global_derivative_amount'])[:2 if B == 9 else 1]:
            jac = torch.eye(2) + 0.3 * torch.randn(M, 2, 2, generator=g)    # [[du_dx, du_dy], [dv_dx, dv_dy]]
            blocks += [uv - pixel * amount * jac[:, :, 1], uv - pixel * amount * jac[:, :, 0]]
        blocks += [uv + pixel * torch.randn(M, 2, generator=g), uv + pixel * torch.randn(M, 2, generator=g)]
        return torch.stack(blocks)

    uv_fg, uv_bg = mapping(), mapping()
    alpha_raw = (torch.rand(5, M, 1, generator=g) * 2 - 1) * 0.999
    rgb_atlas = torch.rand(2, 3, M, 3, generator=g) * 2 - 1
    a = squash(alpha_raw.double())[:, :, 0]
    near = ((a[0] - a[3]).abs() < KINK) | ((a[0] - a[4]).abs() < KINK) | ((a[0] - 0.5).abs() < KINK)
    for uv in (uv_fg.double(), uv_bg.double()):
        near |= ((uv[B - 2] - uv[0]).norm(dim=1) < KINK * pixel) | ((uv[B - 1] - uv[0]).norm(dim=1) < KINK * pixel)
    dropped = float(near.float().mean())
    assert dropped <= KINK_CAP, dropped
    keep = torch.where(~near)[0][:N]
    assert keep.numel() == N
    return (uv_fg[:, keep].reshape(-1, 2).contiguous(), uv_bg[:, keep].reshape(-1, 2).contiguous(), alpha_raw[:, keep].reshape(-1).contiguous(),
            rgb_atlas[:, :, keep].reshape(-1, 3).contiguous(), dropped)


def grad_error(grads, grads64):
    """E of the gradient rule over the four gradient tensors (a tensor whose fp64 gradient is all zero must be all zero)"""
    worst = 0.0
    for g, g64 in zip(grads, grads64):
        assert g.shape == g64.shape, (g.shape, g64.shape)
        if g64.numel() == 0:
            continue
        top = float(g64.abs().max())
        if top == 0.0:
            assert not bool(g.any())
            continue
        worst = max(worst, float((g.double().cpu() - g64).abs().max()) / top)
    return worst


def values_within_rule(L, L32, L64, N):
    """-> the entries of `losses` that break |L - L64| <= max(4 |L32 - L64|, c 2^-24 |L64|); NaN must meet NaN"""
    bad = []
    for k, name in enumerate(LOSSES):
        v, v32, v64 = float(L[k]), float(L32[k]), float(L64[k])
        if v64 != v64:
            if v == v:
                bad.append((name, v, v32, v64))
            continue
        if not abs(v - v64) <= max(4 * abs(v32 - v64), value_ops(N) * 2.0 ** -24 * abs(v64)):
            bad.append((name, v, v32, v64))
    return bad


# ------------------------------------------------------------------------------------------------
# tiny closed-form "networks" of the golden: elementwise, so a row's bits do not depend on the rows it is evaluated with
# ------------------------------------------------------------------------------------------------
class TinyNets(dict):
    def __init__(self, dtype):
        super().__init__()
        self.gain = {k: torch.ones((), dtype=dtype, requires_grad=True) for k in ('FG_UV_Mapping', 'BG_UV_Mapping', 'F_Alpha', 'F_Atlas')}
        g = self.gain
        self['FG_UV_Mapping'] = lambda x: g['FG_UV_Mapping'] * torch.stack(
            (0.8 * x[:, 0] + 0.05 * torch.sin(3 * x[:, 1] + x[:, 2]), 0.8 * x[:, 1] + 0.05 * torch.cos(2 * x[:, 0] - x[:, 2])), dim=1)
        self['BG_UV_Mapping'] = lambda x: g['BG_UV_Mapping'] * torch.stack(
            (0.7 * x[:, 0] - 0.1 * x[:, 1] + 0.04 * torch.sin(2 * x[:, 2]), 0.75 * x[:, 1] + 0.06 * torch.sin(4 * x[:, 0] + x[:, 2])), dim=1)
        self['F_Alpha'] = lambda x: g['F_Alpha'] * torch.tanh(2 * torch.sin(4 * x[:, 0] + x[:, 1]) + x[:, 2]).unsqueeze(1)
        self['F_Atlas'] = lambda u: g['F_Atlas'] * torch.tanh(torch.stack(
            (torch.sin(5 * u[:, 0] + 1) + torch.cos(3 * u[:, 1]), torch.sin(2 * u[:, 0] - u[:, 1]), torch.cos(4 * u[:, 1] + u[:, 0])), dim=1))


GOLDEN_CASE = dict(W=12, H=8, T=3, N=40, seed=4, derivative_amount=1, global_derivative_amount=3)


# ------------------------------------------------------------------------------------------------
# the step on real networks: parameter gradients and the training loop, restated
# ------------------------------------------------------------------------------------------------
STEP_NETWORKS = ('FG_UV_Mapping', 'BG_UV_Mapping', 'F_Alpha', 'F_Atlas')
FIT = dict(res_x=48, res_y=32, frames=4, iters=20, batch=1024, seed=23, global_until=10)
FIT_TRAIN = dict(TRAIN, global_derivative_amount=8, pretrain_global_rigidity_iter=FIT['global_until'])


def param_nets(models, dtype):
    """-> (name -> callable in `dtype` on the CPU, name -> its leaf parameters: per layer weight, bias; F_Atlas's table last)"""
    from atlas_case import mlp_forward
    import hash_fit_case as hc
    nets, par = {}, {}
    for k, m in models.items():
        p = [q.requires_grad_(True) for pair in zip(*hc._weights(m, dtype)) for q in pair]
        if k == 'F_Atlas':
            table = m.encoder.params.detach().cpu().to(dtype).requires_grad_(True)
            nets[k] = (lambda m, p, table: lambda x: hc.hash_forward_diff(p[0::2], p[1::2], table, m.grid, x, m.skip_layers, m.use_tanh))(m, p, table)
            par[k] = p + [table]
        else:
            nets[k] = (lambda m, p: lambda x: mlp_forward(p[0::2], p[1::2], x, m.pe_type, m.pe_dim, m.skip_layers, m.use_tanh))(m, p)
            par[k] = p
    return nets, par


def module_grads(models):
    """the modules' gradients on the CPU in the order of param_nets"""
    out = []
    for k in STEP_NETWORKS:
        m = models[k]
        out += [q.grad.detach().cpu() for lin in m.hidden for q in (lin.weight, lin.bias)]
        if k == 'F_Atlas':
            out.append(m.encoder.params.grad.detach().cpu())
    return out


def step_param_grads(models, idx, data, train, step, dtype):
    """the parameter gradients of one restated step (the networks called block by block, as the reference does) ->
    (the gradients in module_grads' order, losses [14])"""
    nets, par = param_nets({k: models[k] for k in STEP_NETWORKS}, dtype)
    H, W = data['video_frames'].shape[:2]
    q = Queries.from_data(jif_of(idx, H, W), data, train['derivative_amount'], train['global_derivative_amount'])
    total, loss_dict = step_restated(NetEval(nets, dtype), q, train, step <= train['pretrain_alpha_iter'],
                                     step <= train['pretrain_global_rigidity_iter'], dtype)
    leaves = [p for k in STEP_NETWORKS for p in par[k]]
    return list(torch.autograd.grad(total, leaves)), losses_vector(loss_dict, dtype)


def select_pixels(models, data, train, N, seed, with_global=True):
    """N sampled pixels none of whose query rows has a hidden pre-activation within rounding of zero in any network, as
    atlas_fit_case.select_inputs: of 2 N + 64 candidates a pixel is dropped when some |z| < delta in fp64, delta = 16 x the
    largest fp32-vs-fp64 pre-activation difference; at most half may be dropped -> (idx [N, 1], the dropped share)"""
    import atlas_fit_case as fc
    import hash_fit_case as hc
    from atlas_case import mlp_forward
    H, W = data['video_frames'].shape[:2]
    idx = sample(data, 2 * N + 64, seed)
    b = batch_restated(idx, data, train['derivative_amount'], train['global_derivative_amount'], with_global)
    B, M = b['rows'].shape[0], idx.shape[0]
    rows = b['rows'].reshape(B * M, 3)
    z = {}
    with torch.no_grad():
        for dtype in (torch.float64, torch.float32):
            zs, uv = [], {}
            for k in ('FG_UV_Mapping', 'BG_UV_Mapping'):
                m = models[k]
                zs.append(fc.preactivations(m, rows, dtype).view(B, M, -1))
                ws, bs = hc._weights(m, dtype)
                uv[k] = mlp_forward(ws, bs, rows[:3 * M].to(dtype), m.pe_type, m.pe_dim, m.skip_layers, m.use_tanh)
            zs.append(fc.preactivations(models['F_Alpha'], torch.cat((b['rows'][:3], b['rows'][B - 2:])).reshape(5 * M, 3), dtype).view(5, M, -1))
            a = models['F_Atlas']
            for k, shift in (('FG_UV_Mapping', 0.5), ('BG_UV_Mapping', -0.5)):
                zs.append(hc.preactivations(a, uv[k] * 0.5 + shift, dtype).view(3, M, -1))
            z[dtype] = torch.cat([t.permute(1, 0, 2).reshape(M, -1) for t in zs], dim=1)
    delta = 16 * float((z[torch.float32].double() - z[torch.float64]).abs().max())
    keep = ~(z[torch.float64].abs() < delta).any(dim=1)
    dropped = 1.0 - float(keep.float().mean())
    assert dropped <= 0.5, (dropped, delta)
    idx = idx[keep][:N]
    assert idx.shape[0] == N
    return idx.contiguous(), dropped


def pretrain_mappings(models, iters=400, rows=2048, lr=1e-3, seed=0):
    """FG_UV_Mapping and BG_UV_Mapping fitted to uv = 0.8 xy, which is where pretrain_mapping leaves them before the
    reference's loop starts (torch autograd on the CPU, its own generator): Jacobians near the identity"""
    from atlas_case import mlp_forward
    g = torch.Generator().manual_seed(seed)
    for k in ('FG_UV_Mapping', 'BG_UV_Mapping'):
        m = models[k]
        optimizer = torch.optim.Adam(m.hidden.parameters(), lr=lr)
        for _ in range(iters):
            x = torch.rand(rows, 3, generator=g) * 2 - 1
            uv = mlp_forward([lin.weight for lin in m.hidden], [lin.bias for lin in m.hidden], x, m.pe_type, m.pe_dim, m.skip_layers, m.use_tanh)
            loss = (x[:, :2] * TRAIN['uv_mapping_scale'] - uv).norm(dim=1).mean()
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
        m.zero_grad()
    return models


def toy_training_set(seed=3, real=False, grid=None, pretrained=False):
    """(the five networks on the CPU: hidden 64 at twice the default initialisation, or the reference's widths at the default
    one; a 48 x 32 x 4-frame data_dict)"""
    import atlas_render_case as arc
    models = arc.toy_models(arc.toy_config(hidden=64, real=real), grid=arc.SMALL_GRID if grid is None else grid, seed=seed,
                            weight_scale=1.0 if real else 2.0)
    if pretrained:
        pretrain_mappings(models)
    return models, synthetic_data(FIT['res_x'], FIT['res_y'], FIT['frames'], seed)


def run_fit(models, data, device, **over):
    """atlas_fit.fit_atlas on copies of `models` on `device`, the generator seeded -> (history, last loss_dict, the copies)"""
    import copy
    from videoswap_amd import atlas_fit
    cfg = dict(FIT, **over)
    nets = {k: copy.deepcopy(m).to(device) for k, m in models.items()}
    inverse = nets.pop('FG_UV_Mapping_Inverse')
    torch.manual_seed(cfg['seed'])
    history, last = atlas_fit.fit_atlas(nets, data, FIT_TRAIN, cfg['iters'], batch=cfg['batch'], inverse=inverse)
    nets['FG_UV_Mapping_Inverse'] = inverse
    return history, last, nets


def fit_fp64(models, data):
    """the same steps restated in double precision on the CPU, on the same samples -> (total_loss history, fg_inv_loss history)"""
    H, W, _, T = data['video_frames'].shape
    nets, par = param_nets(models, torch.float64)
    optimizer = torch.optim.Adam([{'params': par[k]} for k in STEP_NETWORKS], lr=FIT_TRAIN['optimizer']['lr'])
    optimizer_inverse = torch.optim.Adam(par['FG_UV_Mapping_Inverse'], lr=FIT_TRAIN['optimizer']['lr'])
    torch.manual_seed(FIT['seed'])
    history, inverse_history = [], []
    for step in range(FIT['iters']):
        idx = torch.randint(T * H * W, (FIT['batch'], 1))
        q = Queries.from_data(jif_of(idx, H, W), data, FIT_TRAIN['derivative_amount'], FIT_TRAIN['global_derivative_amount'])
        total, _ = step_restated(NetEval(nets, torch.float64), q, FIT_TRAIN, step <= FIT_TRAIN['pretrain_alpha_iter'],
                                 step <= FIT_TRAIN['pretrain_global_rigidity_iter'], torch.float64)
        optimizer.zero_grad()
        total.backward()
        optimizer.step()
        xyt_fg = q.rows(0)[q.alpha_gt.squeeze(1) == 1].double()
        with torch.no_grad():
            uv = nets['FG_UV_Mapping'](xyt_fg)
        loss = (nets['FG_UV_Mapping_Inverse'](torch.cat([uv, xyt_fg[:, -1:]], dim=-1)) - xyt_fg).norm(dim=1).mean()
        optimizer_inverse.zero_grad()
        loss.backward()
        optimizer_inverse.step()
        history.append(total.item())
        inverse_history.append(loss.item())
    return history, inverse_history


def history_diff(a, b):
    assert len(a) == len(b)
    return max(abs(x - y) for x, y in zip(a, b))
