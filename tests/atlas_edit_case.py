"""Shared pieces of tests/test_atlas_edit.py (CPU) and tests/test_atlas_edit_gpu.py: a numpy restatement of include/vsx.h
K15 in fp32 or fp64, the scatter-max of the masks, the edit half of evaluate_model written out as the reference loops it
(`ref_edit`), and the CPU stand-in of `ops.atlas_edit`.

As in atlas_render_case.hash_encode, the CELL and the RELEVANCE of a row are decided by the fp32 position in both
precisions (relevance is a step: two precisions that disagree about it are not comparable); the fp64 restatement then
takes its weights from its own fp64 position.  `pos_dtype=np.float32` takes them from the fp32 position instead, and
1 - alpha from fp32 as well: that is what the reference computes (positions and 1 - alpha in fp32 tensors; then numpy,
where an int64 corner minus an fp32 position promotes to fp64), and what the golden pins.
"""
import contextlib

import numpy as np
import torch

import atlas_case
import atlas_render_case as arc

F32 = np.float32
CELLS = ((np.ceil, np.ceil), (np.floor, np.floor), (np.floor, np.ceil), (np.ceil, np.floor))     # (of py, of px), in the reference's order


def positions(uv, box, shift, dtype):
    """uv [N, 2] -> (px, py) in `dtype`: q = uv * 0.5 + shift; p = (q - min) * pixel_size, one rounding per operation"""
    uv = np.asarray(uv).astype(dtype)
    minx, miny, ps = (dtype(v) for v in box)
    qx, qy = uv[:, 0] * dtype(0.5) + dtype(shift), uv[:, 1] * dtype(0.5) + dtype(shift)
    return (qx - minx) * ps, (qy - miny) * ps


def sample(uv, tex, box, shift, dtype, base=None, pos_dtype=None):
    """one layer of K15 -> (colour [N, 3] in `dtype`, relevant bool [N], px32, py32)"""
    tex = np.asarray(tex)
    R, C = tex.shape[0], tex.shape[2]
    px32, py32 = positions(uv, box, shift, F32)
    with np.errstate(invalid='ignore'):
        relevant = (np.floor(px32) >= 0) & (np.floor(py32) >= 0) & (np.ceil(px32) < R) & (np.ceil(py32) < R)
    if (pos_dtype or dtype) == F32:
        px, py = px32.astype(dtype), py32.astype(dtype)
    else:
        px, py = positions(uv, box, shift, dtype)
    fx, fy = np.where(relevant, np.floor(px32), 0).astype(np.int64), np.where(relevant, np.floor(py32), 0).astype(np.int64)
    px, py = np.where(relevant, px, 0), np.where(relevant, py, 0)
    x0, x1, y0, y1 = (np.clip(v, 0, R - 1) for v in (fx, fx + 1, fy, fy + 1))
    wx1, wx0, wy1, wy0 = x1.astype(dtype) - px, px - x0.astype(dtype), y1.astype(dtype) - py, py - y0.astype(dtype)
    t = tex.astype(dtype)
    col = t[y0, x0] * (wx1 * wy1)[:, None] + t[y1, x0] * (wx1 * wy0)[:, None] + t[y0, x1] * (wx0 * wy1)[:, None] \
        + t[y1, x1] * (wx0 * wy0)[:, None]
    if C == 4:
        a = col[:, 3:4]
        col = col[:, :3] * a + np.asarray(base).astype(dtype) * (dtype(1) - a)
    assert col.dtype == dtype
    return col, relevant, px32, py32


def scatter_masks(mask, px32, py32, relevant, values):
    """the four cells of every relevant row of `mask` [R, R] become max(old, value): a TRUE maximum (np.maximum.at),
    where the reference's fancy-indexed assignment keeps the last writer among rows that share a cell"""
    px, py = px32[relevant], py32[relevant]
    for fy, fx in CELLS:
        np.maximum.at(mask, (fy(py).astype(np.int64), fx(px).astype(np.int64)), values)


def edit_rows(uv_fg, uv_bg, alpha, tex_fg, box_fg, tex_bg, box_bg, base_fg=None, base_bg=None, masks=None, dtype=F32,
              pos_dtype=None):
    """K15 on numpy arrays -> (edit, fg, bg [N, 3] in `dtype`, relevant uint8 [N]); masks = (mask_fg, mask_bg) fp32
    arrays (or None each), updated in place"""
    alpha32 = np.asarray(alpha).astype(F32).reshape(-1, 1)
    alpha = np.asarray(alpha).astype(dtype).reshape(-1, 1)
    # the reference forms 1 - alpha in an fp32 tensor before numpy promotes it
    na = (F32(1) - alpha32).astype(dtype) if (pos_dtype or dtype) == F32 else dtype(1) - alpha
    cf, rf, pxf, pyf = sample(uv_fg, tex_fg, box_fg, 0.5, dtype, base_fg, pos_dtype)
    cb, rb, pxb, pyb = sample(uv_bg, tex_bg, box_bg, -0.5, dtype, base_bg, pos_dtype)
    zero = np.zeros_like(cf)
    fg = np.where(rf[:, None], cf * alpha, zero)
    bg = np.where(rb[:, None], cb, zero)
    edit = fg + np.where(rb[:, None], cb * na, zero)
    if masks is not None:
        if masks[0] is not None:
            scatter_masks(masks[0], pxf, pyf, rf, np.asarray(alpha).astype(F32).reshape(-1)[rf])
        if masks[1] is not None:
            scatter_masks(masks[1], pxb, pyb, rb, F32(1))
    return edit, fg, bg, rf.astype(np.uint8) | (rb.astype(np.uint8) << 1)


def ref_edit(models, res_x, res_y, number_of_frames, frames, tex_fg, box_fg, tex_bg, box_bg, dtype):
    """evaluate_model:263-298 and 344-404 as the reference loops them (per frame, 100k-pixel batches), the networks and the
    texture arithmetic in `dtype` -> dict(edit, edited_fg, edited_bg [F, H, W, 3], relevant [F, H, W], alpha, mask_fg, mask_bg)"""
    np_dtype = np.float64 if dtype == torch.float64 else F32
    FG, BG, F_Atlas, F_Alpha = (models[k] for k in ('FG_UV_Mapping', 'BG_UV_Mapping', 'F_Atlas', 'F_Alpha'))
    tex_fg, tex_bg = np.asarray(tex_fg, dtype=F32), np.asarray(tex_bg, dtype=F32)
    n = len(frames)
    edit, efg, ebg = (np.zeros((n, res_y, res_x, 3), np_dtype) for _ in range(3))
    rel = np.zeros((n, res_y, res_x), np.uint8)
    alp = np.zeros((n, res_y, res_x), np_dtype)
    masks = (np.zeros(tex_fg.shape[:2], F32), np.zeros(tex_bg.shape[:2], F32))
    with torch.no_grad():
        for k, ii, jj, xyt in arc.ref_batches(res_x, res_y, number_of_frames, frames):
            uv1, uv2 = arc.ref_forward(FG, xyt, dtype), arc.ref_forward(BG, xyt, dtype)
            alpha = 0.5 * (arc.ref_forward(F_Alpha, xyt, dtype) + 1.0)
            alpha = alpha * 0.99
            alpha = alpha + 0.001
            base1 = base2 = None
            if tex_fg.shape[2] == 4:
                base1 = ((arc.ref_forward(F_Atlas, uv1 * 0.5 + 0.5, dtype) + 1) * 0.5).numpy()
            if tex_bg.shape[2] == 4:
                base2 = ((arc.ref_forward(F_Atlas, uv2 * 0.5 - 0.5, dtype) + 1) * 0.5).numpy()
            e, a, b, r = edit_rows(uv1.numpy(), uv2.numpy(), alpha.numpy(), tex_fg, box_fg, tex_bg, box_bg, base1, base2,
                                   masks, dtype=np_dtype)
            edit[k, ii, jj], efg[k, ii, jj], ebg[k, ii, jj], rel[k, ii, jj] = e, a, b, r
            alp[k, ii, jj] = alpha[:, 0].numpy()
    return dict(edit=torch.from_numpy(edit), edited_fg=torch.from_numpy(efg), edited_bg=torch.from_numpy(ebg),
                relevant=torch.from_numpy(rel), alpha=torch.from_numpy(alp), mask_fg=torch.from_numpy(masks[0]),
                mask_bg=torch.from_numpy(masks[1]))


class EditStandin:
    """`ops.atlas_edit` on the CPU: the fp32 restatement; counts calls and rows; refuses what the entry point refuses"""

    def __init__(self):
        self.calls, self.rows = 0, []

    def __call__(self, uv_fg, uv_bg, alpha, tex_fg, box_fg, tex_bg, box_bg, base_fg=None, base_bg=None, masks=None):
        from videoswap_amd._lib import VsxError
        mask_fg, mask_bg = (None, None) if masks is None else masks
        for name, t in (('uv_fg', uv_fg), ('uv_bg', uv_bg), ('alpha', alpha), ('tex_fg', tex_fg), ('tex_bg', tex_bg),
                        ('base_fg', base_fg), ('base_bg', base_bg), ('mask_fg', mask_fg), ('mask_bg', mask_bg)):
            if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
                raise VsxError(f'{name}: expected a contiguous fp32 tensor')
        N = uv_fg.shape[0]
        if uv_fg.dim() != 2 or uv_fg.shape[1] != 2 or uv_bg.shape != uv_fg.shape or alpha.numel() != N:
            raise VsxError('atlas_edit: uv_fg / uv_bg must be [N, 2] and alpha [N]')
        for name, tex, base, mask in (('foreground', tex_fg, base_fg, mask_fg), ('background', tex_bg, base_bg, mask_bg)):
            if tex.dim() != 3:
                raise VsxError(f'atlas_edit: {name} texture must be [R, R, C]')
            if tex.shape[2] not in (3, 4):
                raise NotImplementedError(f'atlas_edit: {name} texture has {tex.shape[2]} channels (3 = RGB, 4 = RGBA overlay)')
            if tex.shape[0] != tex.shape[1]:
                raise VsxError(f'atlas_edit: {name} texture is {tex.shape[0]} x {tex.shape[1]}, not square')
            if tex.shape[0] < 2:
                raise VsxError(f'atlas_edit: {name} texture resolution {tex.shape[0]} (at least 2)')
            if tex.shape[2] == 4 and base is None:
                raise VsxError(f'atlas_edit: an RGBA {name} texture needs the base colours it is laid over')
            if base is not None and tuple(base.shape) != (N, 3):
                raise VsxError(f'atlas_edit: {name} base must be [{N}, 3]')
            if mask is not None and tuple(mask.shape) != tuple(tex.shape[:2]):
                raise VsxError(f'atlas_edit: {name} mask is {tuple(mask.shape)}, the texture {tuple(tex.shape[:2])}')
        self.calls += 1
        self.rows.append(N)
        np_masks = None if masks is None else tuple(None if m is None else m.numpy() for m in masks)       # shares memory
        out = edit_rows(uv_fg.numpy(), uv_bg.numpy(), alpha.numpy(), tex_fg.numpy(), tuple(float(v) for v in box_fg),
                        tex_bg.numpy(), tuple(float(v) for v in box_bg),
                        None if base_fg is None or tex_fg.shape[2] == 3 else base_fg.numpy(),
                        None if base_bg is None or tex_bg.shape[2] == 3 else base_bg.numpy(), np_masks, dtype=F32)
        return tuple(torch.from_numpy(np.ascontiguousarray(o)) for o in out)


@contextlib.contextmanager
def standin():
    """the network stand-ins of atlas_render_case plus the edit stand-in: yields (coord_mlp, hash, edit)"""
    e = EditStandin()
    with atlas_case.swapped(atlas_edit=e), arc.standin() as (c, h):
        yield c, h, e


def counted():
    """the real `ops.coord_mlp`, `ops.hash_mlp` and `ops.atlas_edit`, counted together"""
    return atlas_case.counted('coord_mlp', 'hash_mlp', 'atlas_edit')
