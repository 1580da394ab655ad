"""Layered-neural-atlas point propagation: the host side of propagate_point_displacement.py (reference :20-126).

A drag of a few semantic points on one keyframe is carried to every frame through a TRAINED atlas: the keyframe point
goes to the canonical (u, v) space with `FG_UV_Mapping`, comes back to every frame with `FG_UV_Mapping_Inverse`, and the
displacement follows through two finite-difference Jacobians; `F_Alpha` decides in which frames the point is visible.
The three networks are plain coordinate MLPs (`IMLP_Hash` with mlp_type 'origin'); each is evaluated by ONE launch of the
fused kernel `ops.coord_mlp` (csrc/atlas.hip), and the propagation is batched over all dragged points and frames: three
launches whatever the number of points P and frames T (the reference makes about ten tiny calls per point).  Per row the
arithmetic is that of the reference's per-point calls.

Rendering (the second half of this file) restates the per-frame body of evaluate_model (videoswap/atlas/evaluate.py):
all five networks of a checkpoint, the texture network `F_Atlas` behind its hash grid (`HashGridMLP`, `ops.hash_mlp`),
give the reconstruction, the alpha matte, the atlas textures and the PSNR.  The hash grid is restated from the published
tiny-cuda-nn algorithm and has NOT been compared with tinycudann.  Editing (the third part) restates the
texture-reading half of evaluate_model (:344-419): the video re-rendered from EDITED texture images through `ops.atlas_edit`
(csrc/atlas_edit.hip).  Fitting (videoswap_amd/atlas_fit.py): a `CoordMLP` switched on with
`differentiable_(True)` has weight and bias gradients (csrc/atlas_bwd.hip), which is what mapping pre-training
(`pretrain_mapping`) and the inverse-mapping fit (`fit_inverse_mapping`) need; a `HashGridMLP` switched on the same way
has gradients for its grid table, its layers and its input, which carries the reconstruction half of the
training step (`reconstruction_losses`, `fit_reconstruction`).  The gradient, rigidity and flow losses of train_atlas.py,
the optical flows of its data loading and train_atlas.py as a drop-in are not in scope.
"""
import json
import math
import os

import numpy as np
import torch
import torch.nn as nn

from . import ops

DELTAX, DELTAY = 0.1, 0.05            # finite-difference steps of compute_Wm's callers, in normalised units
MODEL_NAMES = ('FG_UV_Mapping', 'FG_UV_Mapping_Inverse', 'F_Alpha')


def pack_coord_mlp(weights, biases, hidden_dim, enc_dim, skip_layers=()):
    """nn.Linear weights [out, in] / biases of one network -> the fp32 buffer `ops.coord_mlp` streams (include/vsx.h K13):
    per layer the weight zero-padded to [F, K] (F = hidden_dim, 32 for the last layer; K = hidden columns, then the encoded
    columns padded to a multiple of 8) as [F / 32][K / 8][2][32][4] = W[32 t + i][8 b + 4 h + s], then F floats of bias."""
    encp = (enc_dim + 7) // 8 * 8
    last = len(weights) - 1
    parts = []
    for l, (w, b) in enumerate(zip(weights, biases)):
        w, b = w.detach().to(torch.float32), b.detach().to(torch.float32)
        F = 32 if l == last else hidden_dim
        kh = hidden_dim if l > 0 else 0
        ke = encp if (l == 0 or l in skip_layers) else 0
        if w.shape[1] != kh + (enc_dim if ke else 0) or w.shape[0] > F:
            raise ValueError(f'layer {l}: weight {tuple(w.shape)} does not fit hidden_dim {hidden_dim} / {enc_dim} encoded columns')
        full = torch.zeros(F, kh + ke, dtype=torch.float32, device=w.device)
        full[:w.shape[0], :w.shape[1]] = w
        parts.append(full.view(F // 32, 32, (kh + ke) // 8, 2, 4).permute(0, 2, 3, 1, 4).reshape(-1))
        fb = torch.zeros(F, dtype=torch.float32, device=w.device)
        fb[:b.shape[0]] = b
        parts.append(fb)
    return torch.cat(parts).contiguous()


class _LayerStack(nn.Module):
    """What the two restatements of `IMLP_Hash` share: the constructor arguments as attributes, the `hidden` list of
    nn.Linear layers behind `encoding_dimensions` encoded columns (`_build_hidden`, which a subclass calls once its
    encoding is in place), the packed weights and `forward` around the subclass's `_launch`."""

    def __init__(self, input_dim, output_dim, hidden_dim, pe_type, pe_dim, mlp_type, skip_layers, mlp_layers, use_tanh):
        super().__init__()
        self.input_dim, self.output_dim, self.hidden_dim = int(input_dim), int(output_dim), int(hidden_dim)
        self.pe_type, self.pe_dim, self.mlp_type = pe_type, int(pe_dim), mlp_type
        self.skip_layers, self.mlp_layers, self.use_tanh = [int(i) for i in skip_layers], int(mlp_layers), bool(use_tanh)

    def _build_hidden(self, encoding_dimensions):
        self.encoding_dimensions = int(encoding_dimensions)
        self.hidden = nn.ModuleList()
        for i in range(self.mlp_layers):
            if i == 0:
                k = self.encoding_dimensions
            elif i in self.skip_layers:
                k = self.hidden_dim + self.encoding_dimensions
            else:
                k = self.hidden_dim
            self.hidden.append(nn.Linear(k, self.output_dim if i == self.mlp_layers - 1 else self.hidden_dim, bias=True))
        self._packed = None               # (key, buffer): packed once, again only when a parameter changed or moved

    def packed(self):
        params = [q for lin in self.hidden for q in (lin.weight, lin.bias)]
        key = tuple((q.data_ptr(), q._version, q.device) for q in params)
        if self._packed is None or self._packed[0] != key:
            self._packed = (key, pack_coord_mlp([lin.weight for lin in self.hidden], [lin.bias for lin in self.hidden],
                                                self.hidden_dim, self.encoding_dimensions, self.skip_layers))
        return self._packed[1]

    def forward(self, x):
        lead = x.shape[:-1]
        y = self._launch(x.reshape(-1, self.input_dim).to(torch.float32).contiguous())
        return y.reshape(*lead, self.output_dim)


class CoordMLP(_LayerStack):
    """`IMLP_Hash` (videoswap/atlas/implicit_neural_networks.py:98-195): same constructor arguments, same state-dict keys
    (`hidden.<i>.weight` / `hidden.<i>.bias`); `forward` is one launch of the fused fp32 kernel.  `pe_type:
    hash_encoding` (HashGridMLP implements it) and `mlp_type: tcnn` (tinycudann) are not implemented."""

    def __init__(self, input_dim, output_dim, hidden_dim=256, pe_type='none', pe_dim=10, mlp_type='origin', skip_layers=(),
                 mlp_layers=8, use_tanh=True, fp16=False):
        if pe_type == 'hash_encoding':
            raise NotImplementedError("CoordMLP: pe_type 'hash_encoding' (the tinycudann hash grid of F_Atlas) is not "
                                      "implemented; point propagation does not use it")
        if pe_type not in ('none', 'encoding'):
            raise NotImplementedError(f'CoordMLP: pe_type {pe_type!r}')
        if mlp_type != 'origin':
            raise NotImplementedError(f"CoordMLP: mlp_type {mlp_type!r} is not implemented, only 'origin' (nn.Linear layers)")
        super().__init__(input_dim, output_dim, hidden_dim, pe_type, pe_dim, mlp_type, skip_layers, mlp_layers, use_tanh)
        self._build_hidden(2 * self.input_dim * self.pe_dim if pe_type == 'encoding' else self.input_dim)
        self._differentiable = False

    def differentiable_(self, flag=True):
        """Switch the gradient path on (off by default) -> self.  On, and while grad mode is on and a parameter requires
        grad, `forward` records weight and bias gradients (atlas_fit.CoordMLPFunction); there is none for the input."""
        self._differentiable = bool(flag)
        return self

    def _launch(self, x):
        if self._differentiable and torch.is_grad_enabled() and any(q.requires_grad for q in self.parameters()):
            from .atlas_fit import differentiable_forward
            return differentiable_forward(self, x)
        return ops.coord_mlp(x, self.packed(), self.input_dim, self.output_dim, self.hidden_dim, self.mlp_layers,
                             pe_type=self.pe_type, pe_dim=self.pe_dim, mlp_type=self.mlp_type, skip_layers=self.skip_layers,
                             use_tanh=self.use_tanh)


def load_atlas_config(path):
    """The reference's atlas YAML (options/train_videoswap/*/*/*atlas*.yml) as a plain dict."""
    from .config import load_options
    return load_options(path)


def load_atlas_models(atlas_config, checkpoint_path, device=None, names=MODEL_NAMES):
    """init_atlas_model (propagate_point_displacement.py:59-74) -> {name: module} for `names`: the three networks of the
    propagation by default, all five of a checkpoint with RENDER_MODEL_NAMES (`build_network` picks the class).
    `atlas_config`: the dict or the path of the YAML.  Every other entry of the checkpoint (optimizer state, networks not
    named) is ignored."""
    from . import formats
    if isinstance(atlas_config, (str, os.PathLike)):
        atlas_config = load_atlas_config(atlas_config)
    ckpt = formats._load(checkpoint_path)
    models = {}
    for name in names:
        if name not in atlas_config.get('models', {}):
            raise formats.FormatError(f'atlas config: models.{name} is missing')
        if not isinstance(ckpt, dict) or name not in ckpt:
            raise formats.FormatError(f'{checkpoint_path}: no {name!r} state dict')
        try:
            m = build_network(atlas_config['models'][name])
            m.load_state_dict(ckpt[name])
        except NotImplementedError as e:
            raise NotImplementedError(f'models.{name}: {e}') from e
        except formats.FormatError as e:
            raise formats.FormatError(f'{checkpoint_path}: {name}: {e}') from e
        models[name] = m.to(device) if device is not None else m
    return models


def number_of_frames(atlas_config, num_frames=None):
    """min(max_frames, number of frame files) as load_input_data counts (unwrap_utils.py:43-44), without reading a frame;
    `num_frames` stands in for the file count."""
    ds = atlas_config['datasets']
    if num_frames is None:
        path = ds.get('frame_path')
        if not path or not os.path.isdir(path):
            raise FileNotFoundError(f'datasets.frame_path {path!r} is not a directory: pass --num_frames')
        num_frames = len(os.listdir(path))
    return int(min(int(ds['max_frames']), int(num_frames)))


def compute_Wm(xyt, func, deltax, deltay, return_base=False):
    """[..., 3] -> [..., 2, C]: forward differences of `func` along x and y (reference :20-35).  The three stencil points
    of every row go through `func` in ONE call; `return_base` also hands back func(xyt)."""
    lead = xyt.shape[:-1]
    pts = xyt.unsqueeze(0).repeat(3, *([1] * xyt.dim()))
    pts[1, ..., 0] = xyt[..., 0] + deltax
    pts[2, ..., 1] = xyt[..., 1] + deltay
    uv = func(pts.reshape(-1, xyt.shape[-1])).reshape(3, *lead, -1)
    Wm = torch.stack([(uv[1] - uv[0]) / deltax, (uv[2] - uv[0]) / deltay], dim=-2)
    return (Wm, uv[0]) if return_base else Wm


def propagate_point(source_xy, target_xy, t, number_of_frames, FG_UV_Mapping, FG_UV_Mapping_Inverse, F_Alpha,
                    norm_Scoord_func, norm_Tcoord_func, device):
    """All dragged points at once.  source_xy / target_xy: [P, 2] pixel (x, y) at keyframe t (float64 lists or tensors)
    -> (warp_xy [P, T, 2] normalised, alpha [P, T]).  Three network calls: FG_UV_Mapping on [3 P] rows,
    FG_UV_Mapping_Inverse on [3 P T] rows (the base point is the centre of the stencil), F_Alpha on [P T] rows."""
    T = int(number_of_frames)
    src = torch.as_tensor(source_xy, dtype=torch.float64).reshape(-1, 2)
    tgt = torch.as_tensor(target_xy, dtype=torch.float64).reshape(-1, 2)
    P = src.shape[0]
    # the reference normalises in Python floats (float64) and rounds once to fp32
    xyt = torch.cat([norm_Scoord_func(src), torch.full((P, 1), float(norm_Tcoord_func(t)), dtype=torch.float64)], 1)
    xyt = xyt.to(torch.float32).to(device)
    dx_dy = (norm_Scoord_func(tgt) - norm_Scoord_func(src)).to(torch.float32).to(device)           # [P, 2]

    # stage 1: keyframe point -> canonical space, with its Jacobian
    W_fwd, uv = compute_Wm(xyt, FG_UV_Mapping, DELTAX, DELTAY, return_base=True)                   # [P, 2, 2], [P, 2]
    delta_uv = torch.bmm(dx_dy.unsqueeze(1), W_fwd)                                                # [P, 1, 2]

    # stage 2: canonical point -> every frame: the base coordinate and the inverse Jacobian
    frames = torch.arange(T, device=device).unsqueeze(-1)
    tn = norm_Tcoord_func(frames).to(torch.float32)                                                # [T, 1]
    uvt = torch.cat([uv.unsqueeze(1).expand(P, T, 2), tn.unsqueeze(0).expand(P, T, 1)], dim=-1)    # [P, T, 3]
    W_inv, xyt_pred = compute_Wm(uvt, FG_UV_Mapping_Inverse, DELTAX, DELTAY, return_base=True)     # [P, T, 2, 3], [P, T, 3]
    delta_xy = torch.matmul(delta_uv.unsqueeze(1), W_inv[..., :2]).squeeze(2)                      # [P, T, 2]
    warp_xy = xyt_pred[..., :2] + delta_xy

    # stage 3: visibility at the un-dragged location
    alpha = 0.5 * (F_Alpha(xyt_pred.reshape(P * T, 3)).reshape(P, T) + 1.0)
    return warp_xy, alpha


def propagate_point_sequence(source_point_path, source_tap_path, target_point_path, FG_UV_Mapping, FG_UV_Mapping_Inverse,
                             F_Alpha, larger_dim, number_of_frames, norm_Scoord_func=None, norm_Tcoord_func=None,
                             device=None, return_details=False):
    """propagate_point_sequence (reference :77-126) -> the TAP dict with the dragged tracks replaced.  JSON points are
    [y, x].  A dragged point's whole track becomes [-1, -1]; frames with alpha > 0.5 get round((xy + 1) / 2 * larger_dim)
    (torch.round: half to even).  Points the target file does not name keep their tracks; names only in the target file
    are ignored; point_embedding / point_name2id pass through; rows past `number_of_frames` keep [-1, -1]."""
    from . import formats
    larger_dim, T = int(larger_dim), int(number_of_frames)
    if norm_Scoord_func is None:
        norm_Scoord_func = lambda x: x / (larger_dim / 2) - 1  # noqa: E731
    if norm_Tcoord_func is None:
        norm_Tcoord_func = lambda x: x / (T / 2) - 1  # noqa: E731
    if device is None:
        device = next(FG_UV_Mapping.parameters()).device
    with open(source_point_path, 'r') as fr:
        source_point_dict = json.load(fr)
    keyframe_timestep = int(os.path.splitext(os.path.basename(source_point_path))[0])
    with open(target_point_path, 'r') as fr:
        target_point_dict = json.load(fr)
    source_tap = formats._load(source_tap_path)
    pred_tracks, point_name2id = source_tap['pred_tracks'].clone(), source_tap['point_name2id']
    if T > pred_tracks.shape[0]:
        raise formats.FormatError(f'{source_tap_path}: {pred_tracks.shape[0]} frames of tracks, the atlas has {T}')

    names = [k for k in source_point_dict if k in target_point_dict]
    details = {'names': names}
    if names:
        idx = torch.tensor([int(point_name2id[k]) for k in names])
        src = [[source_point_dict[k][1], source_point_dict[k][0]] for k in names]                  # [y, x] -> (x, y)
        tgt = [[target_point_dict[k][1], target_point_dict[k][0]] for k in names]
        with torch.no_grad():
            warp_xy, alpha = propagate_point(src, tgt, keyframe_timestep, T, FG_UV_Mapping, FG_UV_Mapping_Inverse, F_Alpha,
                                             norm_Scoord_func, norm_Tcoord_func, device)
        pixels = (warp_xy + 1) / 2 * larger_dim                                                    # [P, T, 2], before rounding
        visible = alpha > 0.5
        new = torch.where(visible.unsqueeze(-1), torch.round(pixels), torch.full_like(pixels, -1.0))
        pred_tracks[:, idx, :] = -1
        pred_tracks[:T, idx, :] = new.permute(1, 0, 2).to(pred_tracks.dtype).cpu()
        details.update(pixels=pixels.cpu(), alpha=alpha.cpu())
    out = dict(source_tap)
    out['pred_tracks'] = pred_tracks
    return (out, details) if return_details else out


# ------------------------------------------------------------------------------------------------
# Rendering a trained atlas: the hash-grid texture network and evaluate_model's per-frame body
# ------------------------------------------------------------------------------------------------
RENDER_MODEL_NAMES = ('FG_UV_Mapping', 'BG_UV_Mapping', 'F_Atlas', 'F_Alpha', 'FG_UV_Mapping_Inverse')
# the encoding_config IMLP_Hash hands to tcnn.Encoding (implicit_neural_networks.py:118-127)
HASH_GRID = dict(n_levels=16, n_features_per_level=2, log2_hashmap_size=19, base_resolution=16, per_level_scale=1.38)


def hash_grid_levels(cfg=HASH_GRID):
    """The level table of a HashGrid configuration (include/vsx.h K14, restated from the published tiny-cuda-nn algorithm):
    one dict per level with scale (the fp32 value, as a Python float), res, entries, offset (in entries) and hashed."""
    f32 = np.float32
    cap = 1 << int(cfg['log2_hashmap_size'])
    # fp32 log2f / exp2f as correctly rounded values (numpy's own float32 log2 is an ulp off where the C library's is not)
    log_scale = f32(math.log2(float(f32(cfg['per_level_scale']))))
    levels, offset = [], 0
    for l in range(int(cfg['n_levels'])):
        scale = f32(f32(2.0 ** float(f32(l) * log_scale)) * f32(cfg['base_resolution']) - f32(1))
        res = int(math.ceil(float(scale))) + 1
        entries = min((res * res + 7) // 8 * 8, cap)
        stride = res                                       # after dimension 0
        if stride <= entries:
            stride = (stride * res) & 0xffffffff           # dimension 1, uint32
        levels.append(dict(scale=float(scale), res=res, entries=entries, offset=offset, hashed=entries < stride))
        offset += entries
    return levels


def hash_grid_floats(cfg=HASH_GRID):
    """length of the flat table (`encoder.params`) of a configuration"""
    return sum(lv['entries'] for lv in hash_grid_levels(cfg)) * int(cfg['n_features_per_level'])


class _HashGridParams(nn.Module):
    """holds `params` so that the state-dict key is `encoder.params`, as tcnn.Encoding's"""

    def __init__(self, floats):
        super().__init__()
        self.params = nn.Parameter(torch.empty(floats, dtype=torch.float32).uniform_(-1e-4, 1e-4))    # tcnn's initialisation


class HashGridMLP(_LayerStack):
    """`IMLP_Hash` with pe_type 'hash_encoding', mlp_type 'origin' (the texture network F_Atlas): same constructor
    arguments, same state-dict keys (`encoder.params`: the flat fp32 table; `hidden.<i>.weight` / `hidden.<i>.bias`);
    `forward` is one launch of `ops.hash_mlp`.  `grid` replaces the reference's fixed encoding_config (tests)."""

    def __init__(self, input_dim, output_dim, hidden_dim=256, pe_type='hash_encoding', pe_dim=10, mlp_type='origin',
                 skip_layers=(), mlp_layers=8, use_tanh=True, fp16=False, grid=None):
        if pe_type != 'hash_encoding':
            raise NotImplementedError(f'HashGridMLP: pe_type {pe_type!r} (CoordMLP implements none / encoding)')
        if mlp_type != 'origin':
            raise NotImplementedError(f"HashGridMLP: mlp_type {mlp_type!r} is not implemented, only 'origin' (nn.Linear layers)")
        if fp16:
            raise NotImplementedError('HashGridMLP: fp16: true (a half-precision grid table) is not implemented, only fp32')
        if int(input_dim) != 2:
            raise NotImplementedError(f'HashGridMLP: input_dim {input_dim} (the hash grid is implemented for 2 only)')
        grid = dict(HASH_GRID if grid is None else grid)
        if int(grid['n_features_per_level']) != 2:
            raise NotImplementedError(f"HashGridMLP: n_features_per_level {grid['n_features_per_level']} (only 2)")
        super().__init__(input_dim, output_dim, hidden_dim, pe_type, pe_dim, mlp_type, skip_layers, mlp_layers, use_tanh)
        self.grid = grid
        self.encoder = _HashGridParams(hash_grid_floats(grid))           # before the layers: its place in the state dict
        self._build_hidden(int(grid['n_levels']) * int(grid['n_features_per_level']))
        self._differentiable = False

    def differentiable_(self, flag=True):
        """Switch the gradient path on (off by default) -> self.  On, and while grad mode is on and a parameter or the
        input requires grad, `forward` records gradients for the grid table, the layers and the input
        (atlas_fit.HashGridMLPFunction).  The table's gradient is not bit-reproducible from run to run (fp32 atomics)."""
        self._differentiable = bool(flag)
        return self

    def load_state_dict(self, state_dict, *args, **kwargs):
        from . import formats
        table = state_dict.get('encoder.params') if hasattr(state_dict, 'get') else None
        if table is not None and table.numel() != self.encoder.params.numel():
            raise formats.FormatError(
                f'encoder.params holds {table.numel()} values, the hash grid {self.grid} needs {self.encoder.params.numel()} '
                f'(the level table is restated from the tiny-cuda-nn paper, not taken from the library: DESIGN.md §11)')
        if table is not None and table.dtype != torch.float32:
            state_dict = dict(state_dict, **{'encoder.params': table.to(torch.float32)})
        return super().load_state_dict(state_dict, *args, **kwargs)

    def _launch(self, x):
        if self._differentiable and torch.is_grad_enabled() and (x.requires_grad or any(q.requires_grad for q in self.parameters())):
            from .atlas_fit import differentiable_hash_forward
            return differentiable_hash_forward(self, x)
        return ops.hash_mlp(x, self.encoder.params.detach(), self.grid, self.packed(), self.output_dim, self.hidden_dim,
                            self.mlp_layers, skip_layers=self.skip_layers, use_tanh=self.use_tanh)


def build_network(kw, grid=None):
    """models.<name> of an atlas YAML -> the module: `hash_encoding` entries become HashGridMLP (over `grid`, default the
    reference's HASH_GRID), the others CoordMLP."""
    return HashGridMLP(**kw, grid=grid) if kw.get('pe_type') == 'hash_encoding' else CoordMLP(**kw)


def _pixel_axes(res_x, res_y, number_of_frames, device, tensor_time=False):
    """normalised coordinate of every column, row and frame, computed on the CPU as the reference does: integer tensors
    divided in fp32; the time coordinate in Python floats, rounded once to fp32 (evaluate_model: `norm_Tcoord_func(f)`
    times a tensor of ones), or with `tensor_time` as an integer tensor divided and shifted in fp32, two roundings
    (get_mapping_area:160).  The two differ by an ulp where f / (T / 2) is inexact."""
    larger = max(int(res_x), int(res_y))
    xs = torch.arange(int(res_x)) / (larger / 2) - 1
    ys = torch.arange(int(res_y)) / (larger / 2) - 1
    if tensor_time:
        ts = torch.arange(int(number_of_frames)) / (number_of_frames / 2) - 1
    else:
        ts = torch.tensor([f / (number_of_frames / 2) - 1 for f in range(int(number_of_frames))], dtype=torch.float64).to(torch.float32)
    return xs.to(device), ys.to(device), ts.to(device)


def _select_xyt(xs, ys, ts, idx, H, W):
    """rows `idx` of the (frame, row, column) pixel order -> [len(idx), 3] network inputs (selection only)"""
    f, rem = idx // (H * W), idx % (H * W)
    return torch.stack((xs[rem % W], ys[rem // W], ts[f]), dim=1)


def _pixel_chunks(res_x, res_y, number_of_frames, frames, rows_per_call, device):
    """The pixel loop of render_atlas and edit_atlas -> (n, chunks): the number of frames in `frames` (None: all; checked
    here, before anything runs) and an iterator of (r0, r1, xyt) over the n H W pixels in the reference's row order,
    `rows_per_call` at a time across frame borders."""
    W, H, T = int(res_x), int(res_y), int(number_of_frames)
    frames = list(range(T)) if frames is None else [int(f) for f in frames]
    if any(not 0 <= f < T for f in frames):
        raise ValueError(f'frames {frames} outside 0 .. {T - 1}')
    xs, ys, ts = _pixel_axes(W, H, T, device)
    ts = ts[torch.tensor(frames, dtype=torch.long, device=device)] if frames else ts[:0]
    total, step = len(frames) * H * W, int(rows_per_call)

    def chunks():
        for r0 in range(0, total, step):
            r1 = min(r0 + step, total)
            yield r0, r1, _select_xyt(xs, ys, ts, torch.arange(r0, r1, device=device), H, W)
    return len(frames), chunks()


def _mappings_and_alpha(models, xyt):
    """three launches -> (uv_fg [n, 2], uv_bg [n, 2], alpha [n, 1] in 0.001 .. 0.991: evaluate.py:283-285, its three steps)"""
    uv1, uv2, a = models['FG_UV_Mapping'](xyt), models['BG_UV_Mapping'](xyt), models['F_Alpha'](xyt)
    a = 0.5 * (a + 1.0)
    a = a * 0.99
    a = a + 0.001
    return uv1, uv2, a


def _atlas_colours(F_Atlas, uv1, uv2):
    """ONE F_Atlas launch for the foreground and the background queries together -> (rgb_fg, rgb_bg) [n, 3] in [0, 1]"""
    both, n = F_Atlas(torch.cat((uv1 * 0.5 + 0.5, uv2 * 0.5 - 0.5), dim=0)), uv1.shape[0]
    return (both[:n] + 1) * 0.5, (both[n:] + 1) * 0.5


def render_atlas(models, res_x, res_y, number_of_frames, frames=None, rows_per_call=1 << 20):
    """The per-frame body of evaluate_model (evaluate.py:263-298, 406-407) for the frames `frames` (default: all):
    -> dict(reconstruction [F, H, W, 3], alpha [F, H, W], uv_fg [F, H, W, 2], uv_bg [F, H, W, 2], launches) on the
    networks' device.  Pixels go through the networks in the reference's row order, `rows_per_call` at a time across
    frame borders; a chunk costs four launches: FG_UV_Mapping, BG_UV_Mapping, F_Alpha, and ONE F_Atlas launch for the
    foreground and background queries together."""
    device = next(models['FG_UV_Mapping'].parameters()).device
    W, H = int(res_x), int(res_y)
    n, chunks = _pixel_chunks(W, H, number_of_frames, frames, rows_per_call, device)
    rgb, alpha, uv_fg, uv_bg = (torch.empty(n * H * W, c, dtype=torch.float32, device=device) for c in (3, 1, 2, 2))
    launches = 0
    with torch.no_grad():
        for r0, r1, xyt in chunks:
            uv1, uv2, a = _mappings_and_alpha(models, xyt)
            rgb1, rgb2 = _atlas_colours(models['F_Atlas'], uv1, uv2)
            launches += 4
            rgb[r0:r1] = rgb1 * a + rgb2 * (1.0 - a)
            alpha[r0:r1], uv_fg[r0:r1], uv_bg[r0:r1] = a, uv1, uv2
    return dict(reconstruction=rgb.view(n, H, W, 3), alpha=alpha.view(n, H, W), uv_fg=uv_fg.view(n, H, W, 2),
                uv_bg=uv_bg.view(n, H, W, 2), launches=launches)


def atlas_psnr(reconstruction, frames):
    """skimage.metrics.peak_signal_noise_ratio(data_range=1) per frame, as evaluate.py:516-519 uses it, and the mean
    (:591): [F, H, W, 3] values in [0, 1] -> (float64 [F], float)."""
    mse = ((reconstruction.double().cpu() - frames.double().cpu()) ** 2).flatten(1).mean(dim=1)
    psnr = 10 * torch.log10(1.0 / mse)
    return psnr, float(psnr.mean())


def mapping_area(mapping, F_Alpha, res_x, res_y, number_of_frames, uv_shift, masks=None, invert_alpha=False,
                 alpha_thresh=-0.5, rows_per_call=1 << 20):
    """get_mapping_area (evaluate.py:143-187) -> (maxx, minx, maxy, miny, edge_size) as floats: the box of
    `mapping(xyt) * 0.5 + uv_shift` over the pixels of `masks` (bool [T, H, W]; None: every pixel) whose F_Alpha output
    (negated when `invert_alpha`) exceeds `alpha_thresh`.  With the reference's quirks: both pixel axes are normalised
    by the larger side, the box starts as (min 1, max -1) and is clamped to [-1, 1], edge_size is the larger extent."""
    device = next(mapping.parameters()).device
    W, H, T = int(res_x), int(res_y), int(number_of_frames)
    xs, ys, ts = _pixel_axes(W, H, T, device, tensor_time=True)
    if masks is None:
        rows = torch.arange(T * H * W, device=device)
    else:
        rows = torch.nonzero(torch.as_tensor(masks).to(device).reshape(-1), as_tuple=False).reshape(-1)
    lo = torch.tensor([1.0, 1.0], device=device)
    hi = torch.tensor([-1.0, -1.0], device=device)
    with torch.no_grad():
        for r0 in range(0, rows.numel(), int(rows_per_call)):
            xyt = _select_xyt(xs, ys, ts, rows[r0:r0 + int(rows_per_call)], H, W)
            uv, a = mapping(xyt), F_Alpha(xyt).reshape(-1)
            keep = (-a if invert_alpha else a) > alpha_thresh
            if bool(keep.any()):
                uv = uv[keep] * 0.5 + uv_shift
                lo, hi = torch.minimum(lo, uv.min(dim=0).values), torch.maximum(hi, uv.max(dim=0).values)
    (minx, miny), (maxx, maxy) = lo.clamp(min=-1).tolist(), hi.clamp(max=1).tolist()
    return maxx, minx, maxy, miny, max(maxx - minx, maxy - miny)


def atlas_texture(F_Atlas, resolution, minx, maxx, miny, maxy):
    """`texture_orig` of get_high_res_texture (evaluate.py:89-105, without the cv2 annotation): F_Atlas on the
    linspace grid [miny, maxy] x [minx, maxx] -> [resolution, resolution, 3] in [0, 1], one launch."""
    device = next(F_Atlas.parameters()).device
    n = int(resolution)
    indsx = torch.linspace(float(minx), float(maxx), n)
    indsy = torch.linspace(float(miny), float(maxy), n)
    uv = torch.stack((indsx.unsqueeze(0).expand(n, n), indsy.unsqueeze(1).expand(n, n)), dim=-1).reshape(-1, 2)
    with torch.no_grad():
        return 0.5 * (F_Atlas(uv.to(device)).reshape(n, n, 3) + 1)


# ------------------------------------------------------------------------------------------------
# Editing through an atlas: the video re-rendered from edited texture images (evaluate.py:344-419)
# ------------------------------------------------------------------------------------------------
def texture_box(minx, miny, edge, resolution):
    """The box of a texture image as `ops.atlas_edit` takes it: (minx, miny, pixel_size) as Python floats holding fp32
    values.  pixel_size = resolution / ((minx + edge) - minx) is formed in fp32 TENSORS, as the reference forms it
    (get_colors, evaluate.py:65, called with `minx, minx + edge_size` of :222-228), not in doubles rounded afterwards:
    the two differ by an ulp for some boxes, and a position on the edge of a texel follows pixel_size."""
    mx, my, e = (torch.tensor(float(v), dtype=torch.float32) for v in (minx, miny, edge))
    pixel_size = int(resolution) / ((mx + e) - mx)
    return float(mx), float(my), float(pixel_size)


def edit_atlas(models, res_x, res_y, number_of_frames, tex_fg, box_fg, tex_bg, box_bg, frames=None, rows_per_call=1 << 20,
               want_masks=False):
    """The edit half of evaluate_model's per-frame body (evaluate.py:344-404) for the frames `frames` (default: all):
    tex_fg / tex_bg [R, R, 3] replace the atlas textures over the boxes box_fg / box_bg (`texture_box`); with 4 channels a
    texture is an RGBA overlay over the colour F_Atlas gives.  -> dict(edit [F, H, W, 3], edited_fg, edited_bg [F, H, W, 3],
    relevant uint8 [F, H, W] (bit 0 foreground, bit 1 background), alpha [F, H, W], mask_fg, mask_bg ([R, R], the "was this
    texel ever used" images of :373-397, None unless `want_masks`), launches).  Row order and chunking are render_atlas's;
    a chunk costs four launches (FG_UV_Mapping, BG_UV_Mapping, F_Alpha, ops.atlas_edit), five when a texture is RGBA
    (ONE F_Atlas launch gives both base colours).  mask_fg holds the true maximum of alpha per texel; the reference keeps
    the last writer among the rows of one batch that share a texel."""
    device = next(models['FG_UV_Mapping'].parameters()).device
    W, H = int(res_x), int(res_y)
    n, chunks = _pixel_chunks(W, H, number_of_frames, frames, rows_per_call, device)
    tex_fg = torch.as_tensor(tex_fg).to(device=device, dtype=torch.float32).contiguous()
    tex_bg = torch.as_tensor(tex_bg).to(device=device, dtype=torch.float32).contiguous()
    for name, tex in (('tex_fg', tex_fg), ('tex_bg', tex_bg)):
        if tex.dim() != 3 or tex.shape[-1] not in (3, 4):
            raise NotImplementedError(f'edit_atlas: {name} must be [R, R, 3] (a texture) or [R, R, 4] (an RGBA overlay), '
                                      f'got {tuple(tex.shape)}')
    overlay = tex_fg.shape[-1] == 4 or tex_bg.shape[-1] == 4
    masks = None
    if want_masks:
        masks = tuple(torch.zeros(t.shape[0], t.shape[1], dtype=torch.float32, device=device) for t in (tex_fg, tex_bg))
    edit, fg, bg = (torch.empty(n * H * W, 3, dtype=torch.float32, device=device) for _ in range(3))
    relevant = torch.empty(n * H * W, dtype=torch.uint8, device=device)
    alpha = torch.empty(n * H * W, dtype=torch.float32, device=device)
    launches = 0
    with torch.no_grad():
        for r0, r1, xyt in chunks:
            uv1, uv2, a = _mappings_and_alpha(models, xyt)
            a = a.reshape(-1)
            base1, base2 = _atlas_colours(models['F_Atlas'], uv1, uv2) if overlay else (None, None)
            edit[r0:r1], fg[r0:r1], bg[r0:r1], relevant[r0:r1] = ops.atlas_edit(
                uv1, uv2, a, tex_fg, box_fg, tex_bg, box_bg, base_fg=base1 if tex_fg.shape[-1] == 4 else None,
                base_bg=base2 if tex_bg.shape[-1] == 4 else None, masks=masks)
            alpha[r0:r1] = a
            launches += 5 if overlay else 4
    return dict(edit=edit.view(n, H, W, 3), edited_fg=fg.view(n, H, W, 3), edited_bg=bg.view(n, H, W, 3),
                relevant=relevant.view(n, H, W), alpha=alpha.view(n, H, W), mask_fg=masks[0] if masks else None,
                mask_bg=masks[1] if masks else None, launches=launches)


def checkerboard(resolution, squares=10):
    """[resolution, resolution, 3] in {0, 1}: `squares` x `squares` alternating fields, the top-left one white.  Generated,
    not read: the reference's checkerboard.png is not part of this repository."""
    n = int(resolution)
    k = torch.arange(n) * int(squares) // n
    board = ((k.unsqueeze(0) + k.unsqueeze(1)) % 2 == 0).to(torch.float32)
    return board.unsqueeze(-1).expand(n, n, 3).contiguous()


def checkerboard_videos(models, res_x, res_y, number_of_frames, area_fg, area_bg, frames=None, rows_per_call=1 << 20,
                        resolution=500, squares=10):
    """The checkerboard composites of evaluate.py:226-235, 355-361, 415-419: area_fg / area_bg = (minx, miny, edge_size)
    of the foreground and background mapping areas (`mapping_area`); over each, `atlas_texture` at `resolution` is blended
    0.7 : 0.3 with a checkerboard and read back through the mapping networks by `edit_atlas`.
    -> dict(checkerboard_fg = where(relevant, 0.5 (1 - alpha) + fg, 0.5), checkerboard_bg = where(relevant, bg, 0.5),
    both [F, H, W, 3]; texture_fg, texture_bg: the two blended textures; launches)."""
    F_Atlas = models['F_Atlas']
    device = next(F_Atlas.parameters()).device
    board = checkerboard(resolution, squares).to(device)
    texs, boxes = [], []
    for minx, miny, edge in (area_fg, area_bg):
        tex = atlas_texture(F_Atlas, resolution, minx, minx + edge, miny, miny + edge)
        texs.append(board * 0.3 + tex * 0.7)
        boxes.append(texture_box(minx, miny, edge, resolution))
    out = edit_atlas(models, res_x, res_y, number_of_frames, texs[0], boxes[0], texs[1], boxes[1], frames=frames,
                     rows_per_call=rows_per_call)
    rel = out['relevant'].unsqueeze(-1)
    half = torch.full_like(out['edited_fg'], 0.5)
    cfg = torch.where((rel & 1) != 0, 0.5 * (1.0 - out['alpha']).unsqueeze(-1) + out['edited_fg'], half)
    cbg = torch.where((rel & 2) != 0, out['edited_bg'], half)
    return dict(checkerboard_fg=cfg, checkerboard_bg=cbg, texture_fg=texs[0], texture_bg=texs[1], launches=out['launches'] + 2)


from .atlas_fit import (fit_atlas, fit_inverse_mapping, fit_reconstruction, load_mask_frames, pretrain_mapping,  # noqa: E402,F401
                        reconstruction_losses, training_losses)                                                  # (the fitting half)
