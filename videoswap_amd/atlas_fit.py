"""Fitting the networks of a layered neural atlas: the gradient paths of `CoordMLP` and `HashGridMLP`, the two steps of
the reference that need only the first, and the reconstruction half of its training step, which needs both.

`CoordMLP.differentiable_(True)` routes `forward` through `CoordMLPFunction`: `ops.coord_mlp_train_forward` (the forward
kernel, storing its activations) and `ops.coord_mlp_backward` (csrc/atlas_bwd.hip: weight and bias gradients, fp32,
deterministic).  There is no gradient with respect to the input: in train_atlas.py every coordinate network is fed data
coordinates (the inverse's `uv` is computed under no_grad, :257-261); only the hash-grid network F_Atlas needs one.

`HashGridMLP.differentiable_(True)` routes `forward` through `HashGridMLPFunction`: `ops.hash_mlp_train_forward` and
`ops.hash_mlp_backward`: gradients for the grid table `encoder.params`, the layers and the input uv, which
reaches the mapping networks through their outputs.  The table's gradient is a scatter-add with fp32 atomics and is not
bit-reproducible from run to run; everything else is.

`pretrain_mapping` restates videoswap/atlas/unwrap_utils.py:115-138, `fit_inverse_mapping` train_atlas.py:255-266,
`reconstruction_losses` / `fit_reconstruction` train_atlas.py:135-162, 180-196 (the rgb, alpha and sparsity losses),
`training_losses` / `fit_atlas` the whole step and loop of train_atlas.py:127-266 (every network evaluated once
per step on stacked rows, `ops.atlas_batch` for the data gather and `ops.atlas_losses` for every loss and its gradient),
`load_training_data` load_input_data (unwrap_utils.py:42-101).
"""
import os

import numpy as np
import torch

from . import ops


class CoordMLPFunction(torch.autograd.Function):
    """y = module(x) with gradients for the module's `hidden.<i>.weight` / `hidden.<i>.bias` (passed as `params` so that
    autograd sees them); one ops call forward, one backward, whatever the number of rows."""

    @staticmethod
    def forward(ctx, x, module, *params):
        packed = module.packed()
        ctx.net = dict(input_dim=module.input_dim, output_dim=module.output_dim, hidden_dim=module.hidden_dim,
                       mlp_layers=module.mlp_layers, pe_type=module.pe_type, pe_dim=module.pe_dim, mlp_type=module.mlp_type,
                       skip_layers=tuple(module.skip_layers), use_tanh=module.use_tanh)
        ctx.shapes = [tuple(q.shape) for q in params]
        out, saved = ops.coord_mlp_train_forward(x, packed, **ctx.net)
        ctx.save_for_backward(saved, packed)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        saved, packed = ctx.saved_tensors
        grad = ops.coord_mlp_backward(grad_out.contiguous(), saved, packed, **ctx.net)
        views, off = [], 0
        for shape in ctx.shapes:                       # the kernel's order and layout are the parameters' own: views, no copy
            n = int(np.prod(shape))
            views.append(grad[off:off + n].view(shape))
            off += n
        return (None, None, *views)


def differentiable_forward(module, x):
    if x.requires_grad:
        raise NotImplementedError('CoordMLP: input gradients are not implemented (the mapping networks of an atlas take data '
                                  'coordinates; only weight and bias gradients exist)')
    return CoordMLPFunction.apply(x, module, *(q for lin in module.hidden for q in (lin.weight, lin.bias)))


class HashGridMLPFunction(torch.autograd.Function):
    """y = module(x) of a HashGridMLP with gradients for x, for the grid table and for the layers (`table` and `params` are
    passed so that autograd sees them); one ops call forward, one backward, whatever the number of rows.  grad_x is computed
    only when x needs it, the table's gradient only when the table does."""

    @staticmethod
    def forward(ctx, x, table, module, *params):
        packed = module.packed()
        ctx.grid = dict(module.grid)
        ctx.net = dict(output_dim=module.output_dim, hidden_dim=module.hidden_dim, mlp_layers=module.mlp_layers,
                       skip_layers=tuple(module.skip_layers), use_tanh=module.use_tanh)
        ctx.shapes = [tuple(q.shape) for q in params]
        x, table = x.detach(), table.detach()
        out, saved = ops.hash_mlp_train_forward(x, table, ctx.grid, packed, **ctx.net)
        ctx.save_for_backward(x, table, saved, packed)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, table, saved, packed = ctx.saved_tensors
        grad, grad_table, grad_x = ops.hash_mlp_backward(grad_out.contiguous(), x, table, ctx.grid, saved, packed, **ctx.net,
                                                         want_table=ctx.needs_input_grad[1], want_x=ctx.needs_input_grad[0])
        views, off = [], 0
        for shape in ctx.shapes:
            n = int(np.prod(shape))
            views.append(grad[off:off + n].view(shape))
            off += n
        return (grad_x, grad_table, None, *views)


def differentiable_hash_forward(module, x):
    return HashGridMLPFunction.apply(x, module.encoder.params, module, *(q for lin in module.hidden for q in (lin.weight, lin.bias)))


def _norm_funcs(res_x, res_y, number_of_frames):
    larger_dim = max(int(res_x), int(res_y))
    return larger_dim, (lambda x: x / (larger_dim / 2) - 1), (lambda x: x / (number_of_frames / 2) - 1)


class _Differentiable:
    """`differentiable_(True)` on the networks for a block; their earlier setting comes back afterwards"""

    def __init__(self, *modules):
        self.modules = modules

    def __enter__(self):
        self.before = [m._differentiable for m in self.modules]
        for m in self.modules:
            m.differentiable_(True)

    def __exit__(self, *exc):
        for m, flag in zip(self.modules, self.before):
            m.differentiable_(flag)


def pretrain_mapping(model, uv_mapping_scale, res_x, res_y, number_of_frames, pretrain_iters=100, points_per_frame=10000,
                     lr=1e-4, norm_Scoord_func=None, norm_Tcoord_func=None, device=None):
    """pretrain_mapping (unwrap_utils.py:115-138): fit a UV mapping network to `xy * uv_mapping_scale` -> (model, the
    last iteration's loss averaged over the frames).  Adam(lr) with torch's defaults, per frame the reference's two
    `torch.randint` draws (rows, then columns) on the CPU default generator, the loss
    (xyt[:, :2] * scale - uv).norm(dim=1).mean(): with one seed it sees the reference's samples.  The loss that is
    RETURNED is reduced over the rows in double precision (the reference reports the fp32 scalar; a device's fp32
    reduction of 10 000 rows is an ulp or two off, which is as large as the figure's whole fp32-vs-fp64 difference)."""
    T = int(number_of_frames)
    _, norm_s, norm_t = _norm_funcs(res_x, res_y, T)
    norm_s, norm_t = norm_Scoord_func or norm_s, norm_Tcoord_func or norm_t
    device = next(model.parameters()).device if device is None else device
    optimizer = torch.optim.Adam(model.parameters(), lr=lr)
    loss_sum = 0.0
    with _Differentiable(model):
        for it in range(int(pretrain_iters)):
            for f in range(T):
                i_s_int = torch.randint(int(res_y), (int(points_per_frame), 1))
                j_s_int = torch.randint(int(res_x), (int(points_per_frame), 1))
                i_s, j_s = norm_s(i_s_int), norm_s(j_s_int)
                xyt = torch.cat((j_s, i_s, norm_t(f) * torch.ones_like(i_s)), dim=1).to(device)
                uv = model(xyt)
                model.zero_grad()
                loss = (xyt[:, :2] * uv_mapping_scale - uv).norm(dim=1).mean()
                loss.backward()
                optimizer.step()
                if it == int(pretrain_iters) - 1:      # only the last iteration's losses are returned: no host sync before it
                    with torch.no_grad():
                        loss_sum += float((xyt[:, :2].double() * uv_mapping_scale - uv.double()).norm(dim=1).mean())
    return model, loss_sum / T


def load_mask_frames(mask_dir, res_x, res_y, number_of_frames):
    """The masks as load_input_data reads them (unwrap_utils.py:58-69) -> float32 [res_y, res_x, T]: the first T files of
    the sorted directory, PIL 'L' / 255 in float64, resized with cv2.resize's DEFAULT (bilinear) filter — the reference
    passes INTER_NEAREST in the position of `dst`, so it is not in effect.  Foreground is where the value is exactly 1."""
    from PIL import Image
    files = sorted(os.path.join(mask_dir, n) for n in os.listdir(mask_dir))
    if len(files) < number_of_frames:
        raise FileNotFoundError(f'{mask_dir}: {len(files)} mask files, the atlas has {number_of_frames} frames')
    out = torch.zeros(int(res_y), int(res_x), int(number_of_frames))
    for idx in range(int(number_of_frames)):
        mask = np.array(Image.open(files[idx]).convert('L')).astype(np.float64) / 255.
        if mask.shape != (int(res_y), int(res_x)):
            import cv2
            mask = cv2.resize(mask, (int(res_x), int(res_y)))
        out[:, :, idx] = torch.from_numpy(mask)
    return out


def _sample_foreground(n, res_x, res_y, T, norm_s, norm_t, select, device):
    """`n` pixels of the video drawn as train_atlas.py:135-145 draws them (one torch.randint over the (frame, row, column)
    order of get_tuples on the CPU default generator) -> the normalised [m, 3] coordinates of the foreground ones."""
    W, H = int(res_x), int(res_y)
    idx = torch.randint(T * H * W, (int(n), 1))
    f, rem = idx // (H * W), idx % (H * W)
    i, j = rem // W, rem % W
    xyt = torch.cat([norm_s(j), norm_s(i), norm_t(f)], dim=1).to(device)
    if torch.is_tensor(select):
        keep = (select[i.squeeze(1), j.squeeze(1), f.squeeze(1)] == 1).to(device)
    else:
        with torch.no_grad():
            keep = (0.5 * (select(xyt) + 1.0) > 0.5).squeeze(1)
    return xyt[keep]


def _inverse_step(FG_UV_Mapping, FG_UV_Mapping_Inverse, xyt_fg, optimizer):
    """one step of train_atlas.py:257-266 on the foreground rows xyt_fg [m, 3], m > 0 -> the loss (a device scalar)"""
    with torch.no_grad():
        uv_fg = FG_UV_Mapping(xyt_fg)
    inp_uvt_fg = torch.cat([uv_fg, xyt_fg[:, -1:]], dim=-1)
    xyt_pred_fg = FG_UV_Mapping_Inverse(inp_uvt_fg)
    loss = (xyt_pred_fg - xyt_fg).norm(dim=1).mean()
    optimizer.zero_grad()
    loss.backward()
    optimizer.step()
    return loss.detach()


def fit_inverse_mapping(FG_UV_Mapping, FG_UV_Mapping_Inverse, select, res_x, res_y, number_of_frames, iters, batch=10000,
                        lr=1e-4, holdout=4096):
    """The inverse-mapping fit of train_atlas.py:255-266 on its own: per step sample `batch` pixels, keep the foreground
    ones, uv = FG_UV_Mapping(xyt) under no_grad, pred = FG_UV_Mapping_Inverse(cat(uv, t)), loss
    (pred - xyt).norm(dim=1).mean(), one Adam(lr) step.  `select`: the mask frames [res_y, res_x, T]
    (`load_mask_frames`; foreground where 1) or the network F_Alpha (foreground where 0.5 (alpha + 1) > 0.5).  A step
    without a foreground row is skipped.  -> dict(loss_history, steps_skipped, holdout_rows, roundtrip_mean_px,
    roundtrip_max_px): |inverse(uv(x), t) - x| * larger_dim / 2 over the foreground ones of `holdout` further samples (the
    figure the reference prints for one point, :293-300); NaN when none of them is foreground."""
    T = int(number_of_frames)
    larger_dim, norm_s, norm_t = _norm_funcs(res_x, res_y, T)
    device = next(FG_UV_Mapping_Inverse.parameters()).device
    optimizer = torch.optim.Adam(FG_UV_Mapping_Inverse.parameters(), lr=lr)
    history, skipped = [], 0
    with _Differentiable(FG_UV_Mapping_Inverse):
        for _ in range(int(iters)):
            xyt_fg = _sample_foreground(batch, res_x, res_y, T, norm_s, norm_t, select, device)
            if xyt_fg.shape[0] == 0:
                skipped += 1
                continue
            history.append(_inverse_step(FG_UV_Mapping, FG_UV_Mapping_Inverse, xyt_fg, optimizer).item())
    with torch.no_grad():
        xyt = _sample_foreground(holdout, res_x, res_y, T, norm_s, norm_t, select, device)
        mean_px = max_px = float('nan')
        if xyt.shape[0]:
            back = FG_UV_Mapping_Inverse(torch.cat([FG_UV_Mapping(xyt), xyt[:, -1:]], dim=-1))
            err = (back[:, :2] - xyt[:, :2]).norm(dim=1) * (larger_dim / 2)
            mean_px, max_px = float(err.mean()), float(err.max())
    return dict(loss_history=history, steps_skipped=skipped, holdout_rows=int(xyt.shape[0]), roundtrip_mean_px=mean_px,
                roundtrip_max_px=max_px)


# ------------------------------------------------------------------------------------------------
# the reconstruction half of the training step (train_atlas.py:135-162, 180-196)
# ------------------------------------------------------------------------------------------------
NETWORKS = ('FG_UV_Mapping', 'BG_UV_Mapping', 'F_Alpha', 'F_Atlas')
# loss_cfg of the reference's atlas YAMLs, the three weights this half reads
LOSS_CFG = {'reconstruction_loss': {'rgb_loss_weight': 5000.0, 'alpha_loss_weight': 2000.0},
            'sparsity_loss': {'sparsity_loss_weight': 1000.0}}


def reconstruction_losses(models, xyt, rgb, alpha_gt, loss_cfg=None, with_alpha_loss=True):
    """train_atlas.py:147-162, 180-196 without get_gradient_loss -> (loss_total, loss_dict): xyt [n, 3] normalised pixel
    coordinates, rgb [n, 3] their colours, alpha_gt [n, 1] their mask values; `loss_cfg`: train.loss_cfg of the atlas YAML
    (default: the reference's weights); rgb_loss, alpha_loss (`with_alpha_loss`: the reference adds it while global_step
    <= pretrain_alpha_iter) and sparsity_loss, alpha mapped to 0.001 .. 0.991 as there.  F_Atlas is evaluated ONCE on the
    foreground and background queries together, as render_atlas does."""
    from .atlas import _atlas_colours, _mappings_and_alpha
    loss_cfg = LOSS_CFG if loss_cfg is None else loss_cfg
    uv_fg, uv_bg, alpha = _mappings_and_alpha(models, xyt)
    rgb_output_fg, rgb_output_bg = _atlas_colours(models['F_Atlas'], uv_fg, uv_bg)
    rgb_output = rgb_output_fg * alpha + rgb_output_bg * (1.0 - alpha)
    loss_dict = {}
    rgb_loss = (torch.norm(rgb_output - rgb, dim=1) ** 2).mean()
    loss_dict['rgb_loss'] = rgb_loss
    loss_total = loss_cfg['reconstruction_loss']['rgb_loss_weight'] * rgb_loss
    if with_alpha_loss:
        alpha_loss = torch.mean(-alpha_gt * torch.log(alpha) - (1 - alpha_gt) * torch.log(1 - alpha))
        loss_dict['alpha_loss'] = alpha_loss
        loss_total = loss_total + loss_cfg['reconstruction_loss']['alpha_loss_weight'] * alpha_loss
    rgb_loss_sparsity = (torch.norm(rgb_output_fg * (1.0 - alpha), dim=1) ** 2).mean()
    loss_dict['sparsity_loss'] = rgb_loss_sparsity
    loss_total = loss_total + loss_cfg['sparsity_loss']['sparsity_loss_weight'] * rgb_loss_sparsity
    loss_dict['total_loss'] = loss_total
    return loss_total, loss_dict


def fit_reconstruction(models, video_frames, mask_frames, iters, batch=10000, lr=1e-4, train=('F_Atlas',), alpha_loss_iters=None,
                       loss_cfg=None):
    """The reconstruction half of the training loop: video_frames [H, W, 3, T] in [0, 1] and mask_frames [H, W, T] as
    load_input_data holds them (on the CPU, like the reference's), `iters` steps of the reference's sampling
    (train_atlas.py:135-145: one torch.randint over the (frame, row, column) order of get_tuples on the CPU default
    generator, `batch` pixels), `reconstruction_losses`, and ONE Adam(lr) over the networks named in `train` (any of
    FG_UV_Mapping, BG_UV_Mapping, F_Alpha, F_Atlas; the others stay as they are, bit for bit).  With a mapping network in
    `train`, F_Atlas's input gradient drives it.  The alpha loss is added in the steps <= alpha_loss_iters (None: all).
    -> the loss history (total_loss per step)."""
    unknown = [k for k in train if k not in NETWORKS]
    if unknown or not train:
        raise ValueError(f'fit_reconstruction: train {tuple(train)} must name some of {NETWORKS}')
    H, W, _, T = video_frames.shape
    _, norm_s, norm_t = _norm_funcs(W, H, T)
    device = next(models['F_Atlas'].parameters()).device
    before = {k: [q.requires_grad for q in models[k].parameters()] for k in NETWORKS}
    for k in NETWORKS:
        models[k].requires_grad_(k in train)
    optimizer = torch.optim.Adam([q for k in train for q in models[k].parameters()], lr=lr)
    history = []
    try:
        with _Differentiable(*(models[k] for k in NETWORKS)):
            for step in range(int(iters)):
                idx = torch.randint(T * H * W, (int(batch), 1))
                f, rem = idx // (H * W), idx % (H * W)
                i, j = rem // W, rem % W
                rgb = video_frames[i, j, :, f].squeeze(1).to(device=device, dtype=torch.float32)
                alpha_gt = mask_frames[i, j, f].squeeze(1).to(device=device, dtype=torch.float32).unsqueeze(-1)
                xyt = torch.cat([norm_s(j), norm_s(i), norm_t(f)], dim=1).to(device)
                loss, _ = reconstruction_losses(models, xyt, rgb, alpha_gt, loss_cfg,
                                                with_alpha_loss=alpha_loss_iters is None or step <= alpha_loss_iters)
                optimizer.zero_grad()
                loss.backward()
                optimizer.step()
                history.append(loss.item())
    finally:
        for k in NETWORKS:
            for q, flag in zip(models[k].parameters(), before[k]):
                q.requires_grad_(flag)
    return history


# ------------------------------------------------------------------------------------------------
# the full training step (train_atlas.py:127-266)
# ------------------------------------------------------------------------------------------------
# train: of the reference's atlas YAMLs
TRAIN_OPT = {'optimizer': {'type': 'Adam', 'lr': 1e-4}, 'pretrain_alpha_iter': 50000, 'pretrain_global_rigidity_iter': 5000,
             'uv_mapping_scale': 0.8, 'derivative_amount': 1, 'global_derivative_amount': 100,
             'loss_cfg': {'reconstruction_loss': {'rgb_loss_weight': 5000.0, 'gradient_loss_weight': 1000.0, 'alpha_loss_weight': 2000.0},
                          'rigidity_loss': {'rigidity_loss_weight': 1.0, 'global_rigidity_fg_loss_weight': 5.0,
                                            'global_rigidity_bg_loss_weight': 50.0},
                          'flow_loss': {'flow_loss_weight': 5.0, 'alpha_flow_loss_weight': 49.0},
                          'sparsity_loss': {'sparsity_loss_weight': 1000.0}}}
# the keys of the reference's loss_dict in the order it fills them; the two that depend on the step are left out when off
_LOSS_DICT_ORDER = ('gradient_loss', 'rgb_loss', 'alpha_loss', 'alpha_mean_fg', 'alpha_mean_bg', 'sparsity_loss', 'rigidity_loss_fg',
                    'rigidity_loss_bg', 'global_rigidity_loss_fg', 'global_rigidity_loss_bg', 'flow_loss_fg', 'flow_loss_bg',
                    'flow_alpha_loss', 'total_loss')


def loss_kernel_cfg(train_opt, step):
    """the YAML's train section at `step` -> the flat configuration of ops.atlas_losses"""
    cfg = {k: float(v) for group in train_opt['loss_cfg'].values() for k, v in group.items()}
    cfg.update(uv_mapping_scale=float(train_opt['uv_mapping_scale']), derivative_amount=int(train_opt['derivative_amount']),
               global_derivative_amount=int(train_opt['global_derivative_amount']),
               with_alpha_loss=step <= train_opt['pretrain_alpha_iter'])
    return cfg


class AtlasLossFunction(torch.autograd.Function):
    """(total_loss, losses [14]) of the four network outputs of a step (ops.atlas_losses: every loss and the gradient of
    total_loss in one pass); `losses` is not differentiable; backward scales the stored gradients by the incoming scalar"""

    @staticmethod
    def forward(ctx, uv_fg, uv_bg, alpha_raw, rgb_atlas, batch, cfg):
        losses, *grads = ops.atlas_losses(uv_fg.detach().contiguous(), uv_bg.detach().contiguous(), alpha_raw.detach().contiguous(),
                                          rgb_atlas.detach().contiguous(), batch, cfg)
        ctx.save_for_backward(*grads)
        ctx.mark_non_differentiable(losses)
        return losses[11].clone(), losses

    @staticmethod
    def backward(ctx, grad_total, _grad_losses):
        return (*(g * grad_total for g in ctx.saved_tensors), None, None)


def training_losses(models, batch, train_opt, step):
    """One step's losses (train_atlas.py:147-249) on a batch of `ops.atlas_batch` -> (loss_total, loss_dict with the
    reference's keys).  Every network is evaluated ONCE, on its stacked rows: the mapping networks on all B N rows, F_Alpha on
    the blocks 0, 1, 2 and the two flow matches, F_Atlas on the foreground and the background queries of the blocks 0, 1, 2;
    the graph is these four Functions, the uv * 0.5 +- 0.5 with its concatenation, and one loss Function."""
    rows = batch['rows']
    B, N = rows.shape[0], rows.shape[1]
    with_global = step <= train_opt['pretrain_global_rigidity_iter']
    if (B == 9) != with_global:
        raise ValueError(f'training_losses: a batch of {B} blocks at step {step} (pretrain_global_rigidity_iter '
                         f"{train_opt['pretrain_global_rigidity_iter']}: {9 if with_global else 7} blocks)")
    uv_fg = models['FG_UV_Mapping'](rows.view(B * N, 3))
    uv_bg = models['BG_UV_Mapping'](rows.view(B * N, 3))
    alpha_raw = models['F_Alpha'](torch.cat((rows[:3], rows[B - 2:])).view(5 * N, 3))
    rgb_atlas = models['F_Atlas'](torch.cat((uv_fg[:3 * N] * 0.5 + 0.5, uv_bg[:3 * N] * 0.5 - 0.5), dim=0))
    cfg = loss_kernel_cfg(train_opt, step)
    total, losses = AtlasLossFunction.apply(uv_fg, uv_bg, alpha_raw, rgb_atlas, batch, cfg)
    off = set() if cfg['with_alpha_loss'] else {'alpha_loss'}
    if not with_global:
        off |= {'global_rigidity_loss_fg', 'global_rigidity_loss_bg'}
    loss_dict = {k: losses[ops.ATLAS_LOSSES.index(k)] for k in _LOSS_DICT_ORDER if k not in off}
    loss_dict['total_loss'] = total
    return total, loss_dict


def data_to_device(data, device):
    """load_input_data's data_dict on `device`: fp32, contiguous, the reference's layouts (moved ONCE; at 512 x 512 x 72 frames
    the eight arrays are 16 floats per pixel and frame: 1.2 GB)"""
    return {k: data[k].to(device=device, dtype=torch.float32).contiguous() for k in ops.ATLAS_DATA_KEYS}


def fit_atlas(models, data, train_opt, iters, batch=10000, inverse=None, start_step=0, on_step=None):
    """The training loop of train_atlas.py:127-266: `data` = load_input_data's data_dict (`load_training_data`; moved to the
    networks' device once), `train_opt` = the YAML's train section.  Per step: the reference's sampling (one torch.randint
    over the (frame, row, column) order of get_tuples on the CPU default generator: one seed sees the reference's samples),
    `ops.atlas_batch`, `training_losses`, ONE Adam over the four networks with train.optimizer's arguments; with `inverse`
    (FG_UV_Mapping_Inverse) the inverse step of :255-266 on the rows whose alpha_gt is 1 (its compaction is the one host sync
    of a step; a step without such a row is skipped).  The alpha loss runs while step <= pretrain_alpha_iter, the global
    rigidity losses (and their two row blocks) while step <= pretrain_global_rigidity_iter, step = start_step, start_step + 1,
    ...  on_step(step, loss_dict) is called after every step (loss_dict holds device scalars: reading one synchronises).
    -> (the loss history: total_loss per step, the last loss_dict as floats)"""
    device = next(models['F_Atlas'].parameters()).device
    data = data_to_device(data, device)
    H, W, _, T = data['video_frames'].shape
    opt_args = dict(train_opt['optimizer'])
    if opt_args.pop('type', 'Adam') != 'Adam':
        raise NotImplementedError(f"fit_atlas: optimizer {train_opt['optimizer']['type']!r} (the reference knows Adam)")
    optimizer = torch.optim.Adam([{'params': list(models[k].parameters())} for k in NETWORKS], **opt_args)
    optimizer_inverse = None if inverse is None else torch.optim.Adam(inverse.parameters(), **opt_args)
    history, loss_dict = [], {}
    nets = [models[k] for k in NETWORKS] + ([inverse] if inverse is not None else [])
    with _Differentiable(*nets):
        for step in range(int(start_step), int(start_step) + int(iters)):
            idx = torch.randint(T * H * W, (int(batch), 1))
            b = ops.atlas_batch(idx, data, train_opt['derivative_amount'], train_opt['global_derivative_amount'],
                                with_global_rigidity=step <= train_opt['pretrain_global_rigidity_iter'])
            loss, loss_dict = training_losses(models, b, train_opt, step)
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
            if inverse is not None:
                xyt_fg = b['rows'][0][b['alpha_gt'] == 1]
                if xyt_fg.shape[0]:
                    loss_dict['fg_inv_loss'] = _inverse_step(models['FG_UV_Mapping'], inverse, xyt_fg, optimizer_inverse)
            history.append(loss.detach())
            if on_step is not None:
                on_step(step, loss_dict)
    history = torch.stack(history).tolist() if history else []
    return history, {k: float(v.detach()) for k, v in loss_dict.items()}


# ------------------------------------------------------------------------------------------------
# load_input_data (unwrap_utils.py:12-101)
# ------------------------------------------------------------------------------------------------
def _warp_flow(img, flow):
    """warp_flow (unwrap_utils.py:19-25): img [H, W, 2] sampled at (x + flow_x, y + flow_y) -> float64 [H, W, 2].  EXACT
    bilinear interpolation in double precision, samples outside the image counting as 0 (cv2.remap's constant border);
    cv2.remap itself interpolates in fixed point with 5 fractional bits."""
    h, w = flow.shape[:2]
    x = flow[:, :, 0].astype(np.float64) + np.arange(w)
    y = flow[:, :, 1].astype(np.float64) + np.arange(h)[:, np.newaxis]
    finite = np.isfinite(x) & np.isfinite(y)
    x, y = np.where(finite, x, -4.0), np.where(finite, y, -4.0)
    x0, y0 = np.floor(x), np.floor(y)
    wx, wy = x - x0, y - y0
    out = np.zeros((h, w, img.shape[2]), dtype=np.float64)
    for oy, ox, weight in ((0, 0, (1 - wx) * (1 - wy)), (0, 1, wx * (1 - wy)), (1, 0, (1 - wx) * wy), (1, 1, wx * wy)):
        xi, yi = x0 + ox, y0 + oy
        inside = (xi >= 0) & (xi <= w - 1) & (yi >= 0) & (yi <= h - 1)
        xs, ys = np.clip(xi, 0, w - 1).astype(np.int64), np.clip(yi, 0, h - 1).astype(np.int64)
        out += (weight * inside)[:, :, np.newaxis] * img[ys, xs].astype(np.float64)
    return out


def consistency_masks(forward_flow, backward_flow):
    """get_consistency_mask (unwrap_utils.py:12-31): |flow12 + flow21 warped by flow12| < 1, both ways -> two bool [H, W]"""
    def consistent(f12, f21):
        diff = f12.astype(np.float64) + _warp_flow(f21, f12)
        return (diff[:, :, 0] ** 2 + diff[:, :, 1] ** 2) ** .5 < 1.0
    return consistent(forward_flow, backward_flow), consistent(backward_flow, forward_flow)


def load_training_data(datasets_opt):
    """load_input_data (unwrap_utils.py:42-101) -> its data_dict, the same keys and layouts, fp32 on the CPU.  datasets:
    frame_path, mask_path, flow_path, res_x, res_y, max_frames, filter_optical_flow.  The frames go through the loader of
    render_atlas (PIL, bilinear when the size differs), the masks through `load_mask_frames`; video_frames_dx / _dy are the
    forward differences of :71-72; a flow file is a .npy of [2, res_y, res_x, 2] (forward, backward) per frame pair, the first
    T - 1 of the sorted directory.  Flows at another resolution need cv2 (resize_flow) and raise without it.  The
    forward-backward consistency masks use exact bilinear sampling (`consistency_masks`), not cv2.remap."""
    from .render_atlas import IMAGE_EXT, _read_images
    W, H = int(datasets_opt['res_x']), int(datasets_opt['res_y'])
    n_files = len([n for n in os.listdir(datasets_opt['frame_path']) if n.lower().endswith(IMAGE_EXT)])
    T = int(min(int(datasets_opt['max_frames']), n_files))
    video = _read_images(datasets_opt['frame_path'], list(range(T)), (W, H), 'RGB').permute(1, 2, 3, 0).contiguous()    # [H, W, 3, T]
    masks = load_mask_frames(datasets_opt['mask_path'], W, H, T)
    dx, dy = torch.zeros_like(video), torch.zeros_like(video)
    dy[:-1] = video[1:] - video[:-1]
    dx[:, :-1] = video[:, 1:] - video[:, :-1]
    flows, flows_rev = torch.zeros(H, W, 2, T, 1), torch.zeros(H, W, 2, T, 1)
    fmask, rmask = torch.zeros(H, W, T, 1), torch.zeros(H, W, T, 1)
    flow_files = sorted(os.path.join(datasets_opt['flow_path'], n) for n in os.listdir(datasets_opt['flow_path']))
    if len(flow_files) < T - 1:
        raise FileNotFoundError(f"{datasets_opt['flow_path']}: {len(flow_files)} flow files, {T} frames need {T - 1}")
    for idx in range(T - 1):
        flow = np.load(flow_files[idx])
        if flow.ndim != 4 or flow.shape[0] != 2 or flow.shape[3] != 2:
            raise ValueError(f'{flow_files[idx]}: expected [2, H, W, 2] (forward, backward), got {flow.shape}')
        if flow.shape[1] != H or flow.shape[2] != W:
            try:
                import cv2  # noqa: F401
            except ImportError as e:
                raise ImportError(f'{flow_files[idx]}: flows of {flow.shape[2]} x {flow.shape[1]} for an atlas of {W} x {H}: resizing them '
                                  f'(resize_flow, unwrap_utils.py:34-39) needs cv2, which is not installed') from e
            flow = np.stack([_resize_flow(f, H, W) for f in flow])
        forward_flow, backward_flow = flow[0].astype(np.float32), flow[1].astype(np.float32)
        flows[:, :, :, idx, 0] = torch.from_numpy(forward_flow)
        flows_rev[:, :, :, idx + 1, 0] = torch.from_numpy(backward_flow)
        if datasets_opt.get('filter_optical_flow', True):
            m_fwd, m_bwd = consistency_masks(forward_flow, backward_flow)
            fmask[:, :, idx, 0] = torch.from_numpy(m_fwd.astype(np.float32))
            rmask[:, :, idx + 1, 0] = torch.from_numpy(m_bwd.astype(np.float32))
        else:
            fmask[:, :, idx, 0] = 1.0
            rmask[:, :, idx + 1, 0] = 1.0
    return {'video_frames': video, 'mask_frames': masks, 'video_frames_dx': dx, 'video_frames_dy': dy, 'optical_flows': flows,
            'optical_flows_mask': fmask, 'optical_flows_reverse': flows_rev, 'optical_flows_reverse_mask': rmask}


def _resize_flow(flow, newh, neww):
    """resize_flow (unwrap_utils.py:34-39), with its scaling of the x component by the height ratio as it stands there"""
    import cv2
    oldh, oldw = flow.shape[0:2]
    flow = cv2.resize(flow, (neww, newh), interpolation=cv2.INTER_LINEAR)
    flow[:, :, 0] *= newh / oldh
    flow[:, :, 1] *= neww / oldw
    return flow
