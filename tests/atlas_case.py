"""Shared pieces of tests/test_atlas.py (CPU) and tests/test_atlas_gpu.py: a restatement of IMLP_Hash.forward on the
`nn.Linear` layers of a CoordMLP in any dtype, the CPU stand-in of `ops.coord_mlp` (it UNPACKS the kernel's weight
buffer as include/vsx.h K13 describes it, so the packing is under test as well), the fixture of the reference's
propagation, and the comparison rule for tracks."""
import contextlib
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

from util import GOLDEN

FIXTURE = os.path.join(GOLDEN, 'atlas_propagate.pt')
PIXEL_TOL = 2e-3              # values before rounding, in pixels
HALF_BAND, ALPHA_BAND = 0.01, 1e-4
EXCUSED_SHARE = 0.05


def encode(x, pe_dim):
    """positionalEncoding_vec with b = fp32(2^j pi) (the reference's `self.b` is an fp32 tensor), in x's dtype"""
    b = torch.tensor([(2 ** j) * np.pi for j in range(pe_dim)], dtype=torch.float32).to(x.dtype)
    proj = torch.einsum('ij, k -> ijk', x, b)
    mapped = torch.cat((torch.sin(proj), torch.cos(proj)), dim=1)
    return mapped.transpose(2, 1).contiguous().view(mapped.size(0), -1)


def mlp_forward(weights, biases, x, pe_type, pe_dim, skip_layers, use_tanh):
    """IMLP_Hash.forward (mlp_type 'origin') on explicit weights, in the dtype of x"""
    if pe_type == 'encoding':
        x = encode(x, pe_dim)
    inp = x.clone()
    for i, (w, b) in enumerate(zip(weights, biases)):
        if i > 0:
            x = F.relu(x)
        if i in skip_layers:
            x = torch.cat((x, inp), 1)
        x = F.linear(x, w.to(x.dtype), b.to(x.dtype))
    return torch.tanh(x) if use_tanh else x


def ref_forward(mlp, x, dtype):
    """the network of a CoordMLP as a chain of F.linear in `dtype` on the CPU"""
    ws = [lin.weight.detach().cpu() for lin in mlp.hidden]
    bs = [lin.bias.detach().cpu() for lin in mlp.hidden]
    return mlp_forward(ws, bs, x.detach().cpu().to(dtype), mlp.pe_type, mlp.pe_dim, mlp.skip_layers, mlp.use_tanh)


def unpack(packed, input_dim, output_dim, hidden_dim, mlp_layers, pe_type, pe_dim, skip_layers):
    """the inverse of the layout in include/vsx.h K13 -> (weights, biases) with the padding removed"""
    enc = 2 * input_dim * pe_dim if pe_type == 'encoding' else input_dim
    encp = (enc + 7) // 8 * 8
    ws, bs, off = [], [], 0
    for l in range(mlp_layers):
        last = l == mlp_layers - 1
        Fp = 32 if last else hidden_dim
        kh = hidden_dim if l > 0 else 0
        ke = encp if (l == 0 or l in skip_layers) else 0
        K = kh + ke
        w = packed[off:off + Fp * K].view(Fp // 32, K // 8, 2, 32, 4).permute(0, 3, 1, 2, 4).reshape(Fp, K)
        off += Fp * K
        b = packed[off:off + Fp]
        off += Fp
        fo = output_dim if last else hidden_dim
        assert float(w[fo:].abs().sum()) == 0 and float(w[:, kh + (enc if ke else 0):].abs().sum()) == 0   # padding is zero
        ws.append(w[:fo, :kh + (enc if ke else 0)])
        bs.append(b[:fo])
    assert off == packed.numel()
    return ws, bs


class Standin:
    """`ops.coord_mlp` on the CPU in fp32 PyTorch; counts its calls and rows"""

    def __init__(self):
        self.calls, self.rows = 0, []

    def __call__(self, x, packed, input_dim, output_dim, hidden_dim, mlp_layers, pe_type='none', pe_dim=0,
                 mlp_type='origin', skip_layers=(), use_tanh=True):
        if pe_type not in ('none', 'encoding'):
            raise NotImplementedError(f'coord_mlp: pe_type {pe_type!r}')
        if mlp_type != 'origin':
            raise NotImplementedError(f'coord_mlp: mlp_type {mlp_type!r}')
        assert x.dtype == torch.float32 and x.dim() == 2 and x.shape[1] == input_dim and x.is_contiguous()
        self.calls += 1
        self.rows.append(x.shape[0])
        ws, bs = unpack(packed, input_dim, output_dim, hidden_dim, mlp_layers, pe_type, pe_dim, list(skip_layers))
        return mlp_forward(ws, bs, x, pe_type, pe_dim, list(skip_layers), use_tanh)


@contextlib.contextmanager
def swapped(**entries):
    """`ops._raw[name] = entry` for the block; the earlier entries come back afterwards"""
    from videoswap_amd import ops
    saved = {k: ops._raw.get(k) for k in entries}
    ops._raw.update(entries)
    try:
        yield
    finally:
        ops._raw.update(saved)


@contextlib.contextmanager
def counted(*names):
    """the real ops `names` (default: `ops.coord_mlp`), counted together"""
    from videoswap_amd import ops
    box = {'calls': 0}

    def wrap(fn):
        def wrapper(*a, **k):
            box['calls'] += 1
            return fn(*a, **k)
        return wrapper

    with swapped(**{k: wrap(ops._raw[k]) for k in names or ('coord_mlp',)}):
        yield box


@contextlib.contextmanager
def standin():
    s = Standin()
    with swapped(coord_mlp=s):
        yield s


# ------------------------------------------------------------------------------------------------
# the fixture (tests/golden/make_golden_atlas.py) and the comparison rule
# ------------------------------------------------------------------------------------------------
def load_fixture():
    """re-run the reference when its tree is readable, read the recorded file otherwise"""
    import importlib.util
    spec = importlib.util.spec_from_file_location('make_golden_atlas', os.path.join(GOLDEN, 'make_golden_atlas.py'))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    if gen.reference_available():
        return gen.generate(), 'reference'
    return torch.load(FIXTURE, map_location='cpu', weights_only=True), 'fixture'


def build_models(fix, device='cpu'):
    from videoswap_amd.atlas import CoordMLP, MODEL_NAMES
    models = []
    for name in MODEL_NAMES:
        m = CoordMLP(**fix['config']['models'][name])
        m.load_state_dict(fix['state_dicts'][name])
        models.append(m.to(device))
    return models


def write_case(tmp, fix, keep=None):
    """the files propagate_point_sequence reads; `keep`: restrict the TARGET file to these names"""
    src, tgt = os.path.join(tmp, f"{fix['keyframe']:05d}.json"), os.path.join(tmp, 'edit.json')
    tap = os.path.join(tmp, 'TAP.pth')
    target = fix['target_points'] if keep is None else {k: v for k, v in fix['target_points'].items() if k in keep}
    with open(src, 'w') as f:
        json.dump(fix['source_points'], f)
    with open(tgt, 'w') as f:
        json.dump(target, f)
    torch.save({k: (v.clone() if torch.is_tensor(v) else v) for k, v in fix['tap'].items()}, tap)
    return src, tap, tgt


def compare_tracks(fix, out, details, names=None):
    """The rule of the issue.  Values before rounding agree with the reference to 2e-3 pixel; rounded tracks are EQUAL,
    except pairs whose reference value before rounding lies within 0.01 pixel of a half-integer or whose reference alpha
    lies within 1e-4 of 0.5 (one pixel / visibility may differ there); at most 5 % of the compared coordinates may be
    excused.  Returns the figures."""
    T = fix['number_of_frames']
    name2id = fix['tap']['point_name2id']
    dragged = [k for k in fix['source_points'] if k in fix['target_points']]
    names = dragged if names is None else names
    assert details['names'] == names
    ref_tracks, got_tracks = fix['pred_tracks'], out['pred_tracks']
    assert got_tracks.shape == ref_tracks.shape and got_tracks.dtype == ref_tracks.dtype
    compared = excused = 0
    worst_pix = worst_alpha = 0.0
    for j, k in enumerate(names):
        col, p = name2id[k], dragged.index(k)
        ref_pix, ref_alpha = fix['pixels'][p], fix['alpha'][p]                # [T, 2], [T]
        pix, alpha = details['pixels'][j], details['alpha'][j]
        seen = ~torch.isnan(ref_pix)                                          # the reference rounds visible frames only
        if bool(seen.any()):
            worst_pix = max(worst_pix, float((pix - ref_pix)[seen].abs().max()))
        worst_alpha = max(worst_alpha, float((alpha - ref_alpha).abs().max()))
        near_alpha = (ref_alpha - 0.5).abs() <= ALPHA_BAND
        frac = ref_pix - torch.floor(ref_pix)
        near_half = (frac - 0.5).abs() <= HALF_BAND                           # False where the reference has no value
        for t in range(T):
            for c in range(2):
                compared += 1
                r, g = float(ref_tracks[t, col, c]), float(got_tracks[t, col, c])
                if r == g:
                    continue
                ok_alpha = bool(near_alpha[t]) and (r == -1.0 or g == -1.0)
                ok_half = bool(near_half[t, c]) and abs(r - g) == 1.0
                assert ok_alpha or ok_half, (k, t, c, r, g, float(ref_pix[t, c]), float(ref_alpha[t]))
                excused += 1
        assert bool((got_tracks[T:, col] == -1).all())                       # rows past number_of_frames stay cleared
    assert worst_pix <= PIXEL_TOL, worst_pix
    assert excused <= EXCUSED_SHARE * compared, (excused, compared)
    return {'compared': compared, 'excused': excused, 'max_pixel_diff': worst_pix, 'max_alpha_diff': worst_alpha}
