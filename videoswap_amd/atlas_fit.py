"""Fitting the mapping networks of a layered neural atlas: the gradient path of `CoordMLP` and the two steps of the
reference that need nothing else.

`CoordMLP.differentiable_(True)` routes `forward` through `CoordMLPFunction`: `ops.coord_mlp_train_forward` (the forward
kernel, storing its activations) and `ops.coord_mlp_backward` (csrc/atlas_bwd.hip: weight and bias gradients, fp32,
deterministic).  There is no gradient with respect to the input: in train_atlas.py every coordinate network is fed data
coordinates (the inverse's `uv` is computed under no_grad, :257-261); only the hash-grid network F_Atlas needs one, and
that, with the atlas losses, is the half of atlas training that stays out of scope.

`pretrain_mapping` restates videoswap/atlas/unwrap_utils.py:115-138, `fit_inverse_mapping` train_atlas.py:255-266.
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
            with torch.no_grad():
                uv_fg = FG_UV_Mapping(xyt_fg)
            inp_uvt_fg = torch.cat([uv_fg, xyt_fg[:, -1:]], dim=-1)
            xyt_pred_fg = FG_UV_Mapping_Inverse(inp_uvt_fg)
            loss = (xyt_pred_fg - xyt_fg).norm(dim=1).mean()
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
            history.append(loss.item())
    with torch.no_grad():
        xyt = _sample_foreground(holdout, res_x, res_y, T, norm_s, norm_t, select, device)
        mean_px = max_px = float('nan')
        if xyt.shape[0]:
            back = FG_UV_Mapping_Inverse(torch.cat([FG_UV_Mapping(xyt), xyt[:, -1:]], dim=-1))
            err = (back[:, :2] - xyt[:, :2]).norm(dim=1) * (larger_dim / 2)
            mean_px, max_px = float(err.mean()), float(err.max())
    return dict(loss_history=history, steps_skipped=skipped, holdout_rows=int(xyt.shape[0]), roundtrip_mean_px=mean_px,
                roundtrip_max_px=max_px)
