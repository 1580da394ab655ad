"""Records tests/golden/atlas_propagate.pt: the reference's point propagation (propagate_point_displacement.py,
propagate_point_sequence with IMLP_Hash networks) on seeded networks, on the CPU.

    python tests/golden/make_golden_atlas.py

The reference's two files are IMPORTED from its tree (VIDEOSWAP_REFERENCE, default /root/reference), never copied; the
modules they import but propagation never uses (tinycudann, omegaconf, the atlas data loader, the visualiser) are stubbed
in sys.modules for the duration of the import, and the module global `device`, which only the reference's __main__
defines, is set to 'cpu'.  Recorded: the state dicts of the three networks (hidden_dim 64; 6 / 6 / 8 layers; F_Alpha
with pe_type encoding, pe_dim 5), the point files, the input TAP (longer than number_of_frames, two points the target
file does not name, one name only the target file has), the reference's output tracks, the pixel values BEFORE rounding
(torch.round is wrapped; NaN where the reference never rounded, i.e. invisible frames) and the alphas (F_Alpha is
wrapped).  F_Alpha's last bias is shifted so that both visibility branches occur.  `variants`: IMLP_Hash itself on probe
rows, for small networks over pe_type none / encoding, with and without skip layers and tanh.
"""
import contextlib
import importlib.util
import json
import os
import sys
import tempfile
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE_ROOT = os.environ.get('VIDEOSWAP_REFERENCE', '/root/reference')
OUT = os.path.join(HERE, 'atlas_propagate.pt')

HIDDEN, T, T_TAP, RES_X, RES_Y, KEYFRAME = 64, 24, 30, 768, 448, 5
MODELS = {
    'FG_UV_Mapping': dict(input_dim=3, output_dim=2, hidden_dim=HIDDEN, pe_type='none', pe_dim=4, mlp_type='origin',
                          mlp_layers=6, skip_layers=[]),
    'FG_UV_Mapping_Inverse': dict(input_dim=3, output_dim=3, hidden_dim=HIDDEN, pe_type='none', pe_dim=4, mlp_type='origin',
                                  mlp_layers=6, skip_layers=[]),
    'F_Alpha': dict(input_dim=3, output_dim=1, hidden_dim=HIDDEN, pe_type='encoding', pe_dim=5, mlp_type='origin',
                    mlp_layers=8, skip_layers=[]),
}
GAIN = {'FG_UV_Mapping': 2.0, 'FG_UV_Mapping_Inverse': 2.0, 'F_Alpha': 2.2}     # livelier than the default initialisation
_STUBBED = ('tinycudann', 'omegaconf', 'videoswap', 'videoswap.atlas', 'videoswap.atlas.unwrap_utils', 'videoswap.utils',
            'videoswap.utils.vis_util', 'videoswap.atlas.implicit_neural_networks')


def reference_available():
    if not os.path.isfile(os.path.join(REFERENCE_ROOT, 'propagate_point_displacement.py')):
        return False
    try:
        import einops  # noqa: F401  (the reference's propagation uses einops.repeat)
        import tqdm  # noqa: F401
    except ImportError:
        return False
    return True


@contextlib.contextmanager
def reference_modules():
    """(propagate_point_displacement, implicit_neural_networks) of the reference, sys.modules restored afterwards"""
    saved = {k: sys.modules.get(k) for k in _STUBBED}
    dont = sys.dont_write_bytecode
    sys.dont_write_bytecode = True

    def stub(name, path=None, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        if path is not None:
            m.__path__ = path
        sys.modules[name] = m

    try:
        stub('tinycudann')
        stub('omegaconf', OmegaConf=object)
        stub('videoswap', path=[os.path.join(REFERENCE_ROOT, 'videoswap')])
        stub('videoswap.atlas', path=[os.path.join(REFERENCE_ROOT, 'videoswap', 'atlas')])
        stub('videoswap.atlas.unwrap_utils', load_input_data=None)
        stub('videoswap.utils', path=[])
        stub('videoswap.utils.vis_util', visualize_point_sequence=None)
        sys.modules.pop('videoswap.atlas.implicit_neural_networks', None)
        spec = importlib.util.spec_from_file_location('_ref_propagate_point_displacement',
                                                      os.path.join(REFERENCE_ROOT, 'propagate_point_displacement.py'))
        ppd = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(ppd)
        ppd.device = 'cpu'
        yield ppd, sys.modules['videoswap.atlas.implicit_neural_networks']
    finally:
        sys.dont_write_bytecode = dont
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def variant_specs():
    """small networks over the options of IMLP_Hash that the kernel implements"""
    specs = []
    for pe_type in ('none', 'encoding'):
        for skip in ([], [2, 4]):
            for use_tanh in (True, False):
                specs.append(dict(input_dim=2 if skip else 3, output_dim=3 if use_tanh else 2, hidden_dim=32, pe_type=pe_type,
                                  pe_dim=3, mlp_type='origin', mlp_layers=6, skip_layers=skip, use_tanh=use_tanh))
    return specs


def _variants(inn):
    """[{kwargs, state_dict, x, y}]: the reference's IMLP_Hash on 37 probe rows per variant"""
    out = []
    for i, kw in enumerate(variant_specs()):
        torch.manual_seed(100 + i)
        m = inn.IMLP_Hash(**kw).eval()
        x = torch.rand(37, kw['input_dim']) * 2 - 1
        with torch.no_grad():
            y = m(x)
        out.append({'kwargs': kw, 'state_dict': {k: v.clone() for k, v in m.state_dict().items()}, 'x': x, 'y': y.clone()})
    return out


def _points(seed):
    g = torch.Generator().manual_seed(seed)

    def ri(lo, hi):
        return float(torch.randint(lo, hi, (1,), generator=g))

    names = [f'p{i}' for i in range(8)]
    source = {n: [ri(40, RES_Y - 40), ri(40, RES_X - 40)] for n in names}                     # [y, x]
    target = {n: [source[n][0] + ri(-30, 30), source[n][1] + ri(-30, 30)] for n in names[:6]}  # p6, p7 are not dragged
    target['ghost'] = [10.0, 10.0]                                                             # a name only the target file has
    tap = {'pred_tracks': torch.rand(T_TAP, 8, 2, generator=g) * 400,
           'point_name2id': {n: (i * 3) % 8 for i, n in enumerate(names)},                     # columns in another order than names
           'point_embedding': torch.randn(8, 16, generator=g)}
    return source, target, tap


def _run(seed, alpha_shift):
    with reference_modules() as (ppd, inn):
        torch.manual_seed(seed)
        nets = {}
        for name, kw in MODELS.items():
            m = inn.IMLP_Hash(**kw)
            with torch.no_grad():
                for lin in m.hidden:
                    lin.weight.mul_(GAIN[name])
                    lin.bias.mul_(GAIN[name])
            nets[name] = m.eval()
        with torch.no_grad():
            nets['F_Alpha'].hidden[-1].bias.add_(alpha_shift)
        variants = _variants(inn)
        source, target, tap = _points(seed + 1)
        rounded, alphas = [], []
        real_round = torch.round

        def spy_round(x):
            rounded.append(float(x))
            return real_round(x)

        class SpyAlpha(torch.nn.Module):
            def __init__(self, m):
                super().__init__()
                self.m = m

            def forward(self, x):
                y = self.m(x)
                alphas.append(0.5 * (y.detach().clone().flatten() + 1.0))
                return y

        larger = max(RES_X, RES_Y)
        with tempfile.TemporaryDirectory() as d:
            src, tgt, tp = os.path.join(d, f'{KEYFRAME:05d}.json'), os.path.join(d, 'edit.json'), os.path.join(d, 'TAP.pth')
            with open(src, 'w') as f:
                json.dump(source, f)
            with open(tgt, 'w') as f:
                json.dump(target, f)
            torch.save({k: (v.clone() if torch.is_tensor(v) else v) for k, v in tap.items()}, tp)
            torch.round = spy_round
            try:
                with torch.no_grad():
                    out = ppd.propagate_point_sequence(src, tp, tgt, nets['FG_UV_Mapping'], nets['FG_UV_Mapping_Inverse'],
                                                       SpyAlpha(nets['F_Alpha']), larger, T,
                                                       (lambda x: x / (larger / 2) - 1), (lambda x: x / (T / 2) - 1))
            finally:
                torch.round = real_round
    alpha = torch.stack(alphas)                                               # [dragged points in source order, T]
    pixels = torch.full((alpha.shape[0], T, 2), float('nan'))
    it = iter(rounded)
    for p in range(alpha.shape[0]):
        for t in range(T):
            if alpha[p, t] > 0.5:
                pixels[p, t, 0], pixels[p, t, 1] = next(it), next(it)
    assert next(it, None) is None
    return {
        'config': {'models': MODELS, 'datasets': {'res_x': RES_X, 'res_y': RES_Y, 'max_frames': T}},
        'state_dicts': {n: {k: v.clone() for k, v in m.state_dict().items()} for n, m in nets.items()},
        'source_points': source, 'target_points': target, 'keyframe': KEYFRAME, 'number_of_frames': T, 'tap': tap,
        'pred_tracks': out['pred_tracks'].clone(), 'pixels': pixels, 'alpha': alpha, 'seed': seed, 'alpha_shift': alpha_shift,
        'variants': variants,
    }


def shares(fix):
    """(visible share, share of the compared coordinates that the comparison rule could excuse) by the reference's values"""
    alpha, pixels = fix['alpha'], fix['pixels']
    near_alpha = ((alpha - 0.5).abs() <= 1e-4).unsqueeze(-1).expand_as(pixels)
    near_half = ((pixels - torch.floor(pixels)) - 0.5).abs() <= 0.01
    return float((alpha > 0.5).float().mean()), float((near_alpha | near_half).float().mean())


def generate():
    """the first (seed, shift) for which at least a quarter of the (point, frame) pairs fall on each side of alpha = 0.5
    and fewer than 5 % of the coordinates could be excused"""
    for seed in range(8):
        for shift in (0.0, -0.25, -0.5, -0.75, -1.0, -1.5):
            fix = _run(seed, shift)
            visible, excusable = shares(fix)
            if 0.25 <= visible <= 0.75 and excusable < 0.05:
                return fix
    raise RuntimeError('no seed gives both visibility branches')


if __name__ == '__main__':
    fix = generate()
    torch.save(fix, OUT)
    print(OUT, os.path.getsize(OUT), 'bytes; seed', fix['seed'], 'alpha shift', fix['alpha_shift'],
          '(visible share, excusable share) =', shares(fix))
