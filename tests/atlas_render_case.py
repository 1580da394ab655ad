"""Shared pieces of tests/test_atlas_render.py (CPU) and tests/test_atlas_render_gpu.py: a torch restatement of the hash
grid of include/vsx.h K14 in fp32 or fp64 (int64 arithmetic masked to 32 bits; the cell is chosen by torch.floor on the
fp32 position in BOTH precisions, so that the two evaluate the same cell), the network behind it, the per-frame body of
evaluate_model written out as the reference loops it (`ref_render`), toy atlases, and the CPU stand-ins of `ops.hash_mlp`
/ `ops.hash_grid` (the stand-in of `ops.coord_mlp` is atlas_case's)."""
import contextlib

import numpy as np
import torch

import atlas_case

M32 = 0xffffffff
SMALL_GRID = dict(n_levels=4, n_features_per_level=2, log2_hashmap_size=8, base_resolution=4, per_level_scale=2.0)


def hash_encode(x, table, cfg, dtype):
    """x [N, 2] (any float dtype), table flat fp32 -> [N, 2 * n_levels] in `dtype`"""
    from videoswap_amd.atlas import hash_grid_levels
    x32 = x.detach().cpu().to(torch.float32)
    xd = x.detach().cpu().to(dtype)
    tab = table.detach().cpu().view(-1, 2).to(dtype)
    cols = []
    for lv in hash_grid_levels(cfg):
        scale = torch.tensor(lv['scale'], dtype=torch.float32)
        cell = torch.floor(scale * x32 + 0.5)                         # fp32 position decides the cell in both precisions
        pos = scale.to(dtype) * xd + 0.5
        w = pos - cell.to(dtype)
        g = cell.to(torch.int64) & M32                                # (uint32)(int)floorf
        acc = torch.zeros(x32.shape[0], 2, dtype=dtype)
        for c in range(4):
            c0, c1 = (g[:, 0] + (c & 1)) & M32, (g[:, 1] + (c >> 1)) & M32
            if lv['hashed']:
                idx = c0 ^ ((c1 * 2654435761) & M32)
            else:
                idx = (c0 + c1 * lv['res']) & M32
            idx = idx % lv['entries'] + lv['offset']
            weight = (w[:, 0] if c & 1 else 1 - w[:, 0]) * (w[:, 1] if c >> 1 else 1 - w[:, 1])
            acc = acc + weight.unsqueeze(1) * tab[idx]
        cols.append(acc)
    return torch.cat(cols, dim=1)


def hash_forward(weights, biases, table, cfg, x, skip_layers, use_tanh, dtype):
    enc = hash_encode(x, table, cfg, dtype)
    return atlas_case.mlp_forward(weights, biases, enc, 'none', 0, list(skip_layers), use_tanh)


def ref_forward(m, x, dtype):
    """a CoordMLP or HashGridMLP as torch in `dtype` on the CPU"""
    from videoswap_amd.atlas import HashGridMLP
    if not isinstance(m, HashGridMLP):
        return atlas_case.ref_forward(m, x, dtype)
    ws = [lin.weight.detach().cpu() for lin in m.hidden]
    bs = [lin.bias.detach().cpu() for lin in m.hidden]
    return hash_forward(ws, bs, m.encoder.params, m.grid, x, m.skip_layers, m.use_tanh, dtype)


def ref_batches(res_x, res_y, number_of_frames, frames):
    """the pixels of evaluate_model:263-282 as the reference loops them (per frame, torch.where over the image, 100k-pixel
    batches): yields (k, ii, jj, xyt) with frames[k] the frame, ii / jj the rows / columns, xyt [n, 3] the fp32 inputs"""
    larger = np.maximum(np.int64(res_x), np.int64(res_y))
    norm_s = lambda v: v / (larger / 2) - 1  # noqa: E731
    norm_t = lambda v: v / (number_of_frames / 2) - 1  # noqa: E731
    for k, f in enumerate(frames):
        relis_i, reljs_i = torch.where(torch.ones(res_y, res_x) > 0)
        parts = int(np.ceil(relis_i.shape[0] / 100000))
        for ii, jj in zip(np.array_split(relis_i.numpy(), parts), np.array_split(reljs_i.numpy(), parts)):
            relis = norm_s(torch.from_numpy(ii).unsqueeze(1))
            reljs = norm_s(torch.from_numpy(jj).unsqueeze(1))
            xyt = torch.cat((reljs, relis, norm_t(f) * torch.ones_like(relis)), dim=1)
            assert xyt.dtype == torch.float32
            yield k, ii, jj, xyt


def ref_render(models, res_x, res_y, number_of_frames, frames, dtype):
    """evaluate_model:263-298 as the reference loops it (`ref_batches`), the networks in `dtype`
    -> reconstruction [F, H, W, 3], alpha [F, H, W], uv_fg, uv_bg"""
    FG, BG, F_Atlas, F_Alpha = (models[k] for k in ('FG_UV_Mapping', 'BG_UV_Mapping', 'F_Atlas', 'F_Alpha'))
    rec = torch.zeros(len(frames), res_y, res_x, 3, dtype=dtype)
    alp = torch.zeros(len(frames), res_y, res_x, dtype=dtype)
    uvf, uvb = torch.zeros(len(frames), res_y, res_x, 2, dtype=dtype), torch.zeros(len(frames), res_y, res_x, 2, dtype=dtype)
    with torch.no_grad():
        for k, ii, jj, xyt in ref_batches(res_x, res_y, number_of_frames, frames):
            uv1, uv2 = ref_forward(FG, xyt, dtype), ref_forward(BG, xyt, dtype)
            rgb1 = (ref_forward(F_Atlas, uv1 * 0.5 + 0.5, dtype) + 1) * 0.5
            rgb2 = (ref_forward(F_Atlas, uv2 * 0.5 - 0.5, dtype) + 1) * 0.5
            alpha = 0.5 * (ref_forward(F_Alpha, xyt, dtype) + 1.0)
            alpha = alpha * 0.99
            alpha = alpha + 0.001
            rec[k, ii, jj] = rgb1 * alpha + rgb2 * (1.0 - alpha)
            alp[k, ii, jj] = alpha[:, 0]
            uvf[k, ii, jj], uvb[k, ii, jj] = uv1, uv2
    return dict(reconstruction=rec, alpha=alp, uv_fg=uvf, uv_bg=uvb)


def toy_config(hidden=64, real=False):
    """models.* of an atlas YAML.  real: the widths and depths of the reference's configs (hidden 256, F_Atlas 8 layers with
    skips [4, 7], F_Alpha with the sin/cos encoding)"""
    h = 256 if real else hidden
    mapping = dict(input_dim=3, output_dim=2, hidden_dim=h, pe_type='none', pe_dim=4, mlp_type='origin',
                   mlp_layers=6 if real else 3, skip_layers=[], use_tanh=True, fp16=False)
    return {'FG_UV_Mapping': dict(mapping), 'BG_UV_Mapping': dict(mapping, mlp_layers=4),
            'FG_UV_Mapping_Inverse': dict(mapping, output_dim=3),
            'F_Alpha': dict(mapping, output_dim=1, pe_type='encoding', pe_dim=5, mlp_layers=8 if real else 3),
            'F_Atlas': dict(input_dim=2, output_dim=3, hidden_dim=h, pe_type='hash_encoding', pe_dim=10, mlp_type='origin',
                            mlp_layers=8 if real else 4, skip_layers=[4, 7] if real else [2], use_tanh=True, fp16=False)}


def toy_models(config, grid=SMALL_GRID, seed=0, weight_scale=2.0, table_range=0.5, device='cpu'):
    """{name: module} with weights at `weight_scale` x the nn.Linear default initialisation and a grid table uniform in
    [-table_range, table_range] (a texture that varies visibly); grid None: the reference's configuration"""
    from videoswap_amd.atlas import build_network
    torch.manual_seed(seed)
    models = {}
    for name, kw in config.items():
        m = build_network(kw, grid=grid)
        with torch.no_grad():
            for lin in m.hidden:
                lin.weight.mul_(weight_scale)
                lin.bias.mul_(weight_scale)
            if kw['pe_type'] == 'hash_encoding':
                m.encoder.params.uniform_(-table_range, table_range)
        models[name] = m.to(device)
    return models


class HashStandin:
    """`ops.hash_mlp` / `ops.hash_grid` on the CPU in fp32 PyTorch (weights UNPACKED from the kernel's buffer); counts calls"""

    def __init__(self):
        self.calls, self.rows = 0, []

    def hash_grid(self, x, table, grid):
        assert x.dtype == torch.float32 and x.dim() == 2 and x.is_contiguous() and table.dim() == 1
        if x.shape[1] != 2:
            raise NotImplementedError(f'hash_grid: input_dim {x.shape[1]}')
        return hash_encode(x, table, grid, torch.float32)

    def hash_mlp(self, x, table, grid, packed, output_dim, hidden_dim, mlp_layers, skip_layers=(), use_tanh=True):
        enc = self.hash_grid(x, table, grid)
        self.calls += 1
        self.rows.append(x.shape[0])
        ws, bs = atlas_case.unpack(packed, enc.shape[1], output_dim, hidden_dim, mlp_layers, 'none', 0, list(skip_layers))
        return atlas_case.mlp_forward(ws, bs, enc, 'none', 0, list(skip_layers), use_tanh)


@contextlib.contextmanager
def standin():
    """both stand-ins: yields (the coord_mlp stand-in, the hash stand-in)"""
    h = HashStandin()
    with atlas_case.swapped(hash_mlp=h.hash_mlp, hash_grid=h.hash_grid), atlas_case.standin() as c:
        yield c, h


def counted():
    """the real `ops.coord_mlp` and `ops.hash_mlp`, counted together"""
    return atlas_case.counted('coord_mlp', 'hash_mlp')
