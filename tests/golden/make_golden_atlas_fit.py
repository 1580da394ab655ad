"""Records tests/golden/atlas_pretrain.pt: the reference's own pretrain_mapping (videoswap/atlas/unwrap_utils.py:115-138)
on its own IMLP_Hash, on the CPU.

    python tests/golden/make_golden_atlas_fit.py

The reference's two files are IMPORTED from its tree (VIDEOSWAP_REFERENCE, default /root/reference), never copied; the
modules they import but pretrain_mapping never uses (tinycudann, cv2, imageio, PIL) are stubbed in sys.modules for the
duration of the import where they are missing, as make_golden_atlas.py does.  The run is small on purpose: 3 -> 2, hidden 32,
3 layers, pe none, res_x 32, res_y 24, 2 frames, 3 iterations (six Adam steps of 10 000 samples), scale 0.8, three seeds.
Each seed runs once in fp32 and once in fp64 (`model.double()` and double-valued norm functions, which are arguments: the
integer samples are the same).  Recorded per seed: the initial and both final state dicts, both returned losses, and both
final networks' outputs on a fixed 4096-row probe.
"""
import contextlib
import importlib.util
import os
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE_ROOT = os.environ.get('VIDEOSWAP_REFERENCE', '/root/reference')
OUT = os.path.join(HERE, 'atlas_pretrain.pt')

SPEC = dict(input_dim=3, output_dim=2, hidden_dim=32, pe_type='none', pe_dim=4, mlp_type='origin', mlp_layers=3, skip_layers=[])
RES_X, RES_Y, FRAMES, ITERS, SCALE, SEEDS, PROBE_ROWS = 32, 24, 2, 3, 0.8, (0, 1, 2), 4096
_OPTIONAL = ('tinycudann', 'cv2', 'imageio', 'PIL', 'PIL.Image')


def reference_available():
    if not os.path.isfile(os.path.join(REFERENCE_ROOT, 'videoswap', 'atlas', 'unwrap_utils.py')):
        return False
    try:
        import tqdm  # noqa: F401
    except ImportError:
        return False
    return True


@contextlib.contextmanager
def reference_modules():
    """(unwrap_utils, implicit_neural_networks) of the reference, sys.modules restored afterwards"""
    saved = {k: sys.modules.get(k) for k in _OPTIONAL}
    dont = sys.dont_write_bytecode
    sys.dont_write_bytecode = True
    try:
        for name in _OPTIONAL:
            try:
                importlib.import_module(name)
            except ImportError:
                m = types.ModuleType(name)
                if name == 'PIL':
                    m.__path__ = []
                    m.Image = None
                sys.modules[name] = m
        mods = []
        for stem in ('unwrap_utils', 'implicit_neural_networks'):
            spec = importlib.util.spec_from_file_location(f'_ref_{stem}', os.path.join(REFERENCE_ROOT, 'videoswap', 'atlas', f'{stem}.py'))
            mod = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mod)
            mods.append(mod)
        yield tuple(mods)
    finally:
        sys.dont_write_bytecode = dont
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def probe():
    g = torch.Generator().manual_seed(4096)
    return torch.rand(PROBE_ROWS, SPEC['input_dim'], generator=g) * 2 - 1


def _one(uu, inn, seed, double):
    torch.manual_seed(seed)
    model = inn.IMLP_Hash(**SPEC)
    initial = {k: v.clone() for k, v in model.state_dict().items()}
    larger = max(RES_X, RES_Y)
    if double:
        model = model.double()
        norm_s = lambda x: x.double() / (larger / 2) - 1 if torch.is_tensor(x) else x / (larger / 2) - 1  # noqa: E731
        norm_t = lambda f: torch.tensor(f / (FRAMES / 2) - 1, dtype=torch.float64)  # noqa: E731
    else:
        norm_s = lambda x: x / (larger / 2) - 1  # noqa: E731
        norm_t = lambda f: f / (FRAMES / 2) - 1  # noqa: E731
    model, loss = uu.pretrain_mapping(model, SCALE, RES_X, RES_Y, FRAMES, norm_s, norm_t, 'cpu', pretrain_iters=ITERS)
    with torch.no_grad():
        y = model(probe().to(torch.float64 if double else torch.float32))
    return initial, {k: v.clone() for k, v in model.state_dict().items()}, float(loss), y.clone()


def generate():
    runs = []
    with reference_modules() as (uu, inn):
        for seed in SEEDS:
            init, final32, loss32, y32 = _one(uu, inn, seed, False)
            _, final64, loss64, y64 = _one(uu, inn, seed, True)
            runs.append(dict(seed=seed, initial=init, final_fp32=final32, final_fp64=final64, loss_fp32=loss32, loss_fp64=loss64,
                             probe_fp32=y32, probe_fp64=y64))
    return dict(spec=SPEC, res_x=RES_X, res_y=RES_Y, frames=FRAMES, iters=ITERS, scale=SCALE, probe=probe(), runs=runs)


if __name__ == '__main__':
    fix = generate()
    torch.save(fix, OUT)
    d32 = max(float((r['probe_fp32'].double() - r['probe_fp64']).abs().max()) for r in fix['runs'])
    dl = max(abs(r['loss_fp32'] - r['loss_fp64']) for r in fix['runs'])
    print(OUT, os.path.getsize(OUT), 'bytes; fp32 vs fp64 reference: probe', d32, 'loss', dl)
