"""Records tests/golden/atlas_edit.pt: the reference's own `get_colors` (videoswap/atlas/evaluate.py:64-85, with
bilinear_interpolate_numpy :24-45) on seeded rows, and what evaluate_model composes from it.

    python tests/golden/make_golden_atlas_edit.py

evaluate.py is IMPORTED from the reference's tree (VIDEOSWAP_REFERENCE, default /root/reference), never copied; the
modules it imports at its top but get_colors never uses (cv2, imageio, matplotlib, skimage, scipy, its own loss_utils)
are stubbed in sys.modules for the duration of the import.  Recorded, set `colours`: about 300 rows (uv inside and
outside both boxes, alpha in 0.001 .. 0.991), two 16 x 16 RGB textures, the foreground box as evaluate_model passes it
(Python ints 0 and 1) and a background box of fp32 tensors with an inexact edge; per layer the relevance, the positions
and the colours of the relevant rows as get_colors returns them (the colours are FLOAT64: numpy promotes an int64 corner
minus an fp32 position), and edit / edited_fg / edited_bg composed the way evaluate_model:399-404 composes them.
Set `masks`: at most 16 rows whose cells are all distinct, and the two mask images after the fancy-indexed maximum of
evaluate_model:373-397, restated here as one loop over the four (ceil / floor) cell choices; the generator asserts that
no cell is touched twice, which is where the reference's last-writer assignment and a true maximum agree.
"""
import contextlib
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE_ROOT = os.environ.get('VIDEOSWAP_REFERENCE', '/root/reference')
OUT = os.path.join(HERE, 'atlas_edit.pt')
R, N_ROWS, N_MASK = 16, 300, 16
_STUBBED = ('cv2', 'imageio', 'matplotlib', 'matplotlib.image', 'matplotlib.pyplot', 'skimage', 'skimage.measure',
            'skimage.metrics', 'scipy', 'scipy.interpolate', 'videoswap', 'videoswap.atlas', 'videoswap.atlas.loss_utils',
            'videoswap.atlas.evaluate')


def reference_available():
    if not os.path.isfile(os.path.join(REFERENCE_ROOT, 'videoswap', 'atlas', 'evaluate.py')):
        return False
    try:
        import tqdm  # noqa: F401  (imported at the top of evaluate.py)
    except ImportError:
        return False
    return True


@contextlib.contextmanager
def reference_evaluate():
    """videoswap.atlas.evaluate of the reference, sys.modules restored afterwards"""
    saved = {k: sys.modules.get(k) for k in _STUBBED}
    dont = sys.dont_write_bytecode
    sys.dont_write_bytecode = True

    def stub(name, path=None, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        if path is not None:
            m.__path__ = path
        sys.modules[name] = m
        return m

    try:
        for name in ('cv2', 'imageio'):
            stub(name)
        mpl = stub('matplotlib', path=[], use=lambda *a, **k: None)
        mpl.image, mpl.pyplot = stub('matplotlib.image'), stub('matplotlib.pyplot')
        sk = stub('skimage', path=[])
        sk.measure, sk.metrics = stub('skimage.measure'), stub('skimage.metrics')
        stub('scipy', path=[])
        stub('scipy.interpolate', griddata=None)
        stub('videoswap', path=[os.path.join(REFERENCE_ROOT, 'videoswap')])
        stub('videoswap.atlas', path=[os.path.join(REFERENCE_ROOT, 'videoswap', 'atlas')])
        stub('videoswap.atlas.loss_utils', get_optical_flow_alpha_loss_all=None, get_optical_flow_loss_all=None,
             get_rigidity_loss=None)
        sys.modules.pop('videoswap.atlas.evaluate', None)
        yield importlib.import_module('videoswap.atlas.evaluate')
    finally:
        sys.dont_write_bytecode = dont
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def _inputs(seed):
    g = torch.Generator().manual_seed(seed)
    uv_fg = torch.rand(N_ROWS, 2, generator=g) * 2.5 - 1.25                     # [0, 1]^2 needs uv in [-1, 1]: a fifth outside per axis
    uv_bg = torch.rand(N_ROWS, 2, generator=g) * 1.3 - 0.9                      # around the background box below
    alpha = 0.5 * (torch.rand(N_ROWS, 1, generator=g) * 2 - 1 + 1.0)
    alpha = alpha * 0.99
    alpha = alpha + 0.001
    tex_fg, tex_bg = torch.rand(R, R, 3, generator=g), torch.rand(R, R, 3, generator=g)
    # evaluate_model:214-216: the foreground box is Python ints; :217 the background box is 0-d fp32 tensors
    box_fg = (0, 0, 1)
    box_bg = (torch.tensor(-0.73), torch.tensor(-0.81), torch.tensor(0.37))
    return uv_fg, uv_bg, alpha, tex_fg, tex_bg, box_fg, box_bg


def _layer(ev, uv, shift, box, tex):
    minx, miny, edge = box
    rgb, px, py, relevant = ev.get_colors(R, minx, minx + edge, miny, miny + edge, uv[:, 0] * 0.5 + shift, uv[:, 1] * 0.5 + shift, tex)
    return rgb, px, py, relevant


def _mask_rows(ev, tex, box, shift, seed):
    """N_MASK rows inside `box` whose sixteen-cell footprints are pairwise disjoint: one row per 4 x 4 block of texels"""
    g = torch.Generator().manual_seed(seed)
    minx, miny, edge = (float(v) for v in box)
    cells = [(2 + 4 * (k % 4), 2 + 4 * (k // 4)) for k in range(N_MASK)]        # texel (x, y) of the row's floor cell
    frac = torch.rand(N_MASK, 2, generator=g) * 0.8 + 0.1
    pos = (torch.tensor(cells, dtype=torch.float32) + frac) / R * edge + torch.tensor([minx, miny])
    return ((pos - shift) * 2).to(torch.float32)                                # uv with uv * 0.5 + shift = pos


def generate():
    with reference_evaluate() as ev:
        uv_fg, uv_bg, alpha, tex_fg, tex_bg, box_fg, box_bg = _inputs(0)
        fix = {'uv_fg': uv_fg, 'uv_bg': uv_bg, 'alpha': alpha[:, 0].clone(), 'tex_fg': tex_fg, 'tex_bg': tex_bg, 'R': R,
               'area_fg': [float(v) for v in box_fg], 'area_bg': [float(v) for v in box_bg]}
        rgb1, px1, py1, rel1 = _layer(ev, uv_fg, 0.5, box_fg, tex_fg)
        rgb2, px2, py2, rel2 = _layer(ev, uv_bg, -0.5, box_bg, tex_bg)
        assert rgb1.dtype == np.float64 and px1.dtype == np.float32
        a = alpha.numpy()
        edit1, edit2, edit = (np.zeros((N_ROWS, 3)) for _ in range(3))        # evaluate_model:238-242, one pixel per row
        edit1[rel1] = rgb1 * a[rel1]
        edit2[rel2] = rgb2
        edit[rel1] = edit[rel1] + rgb1 * a[rel1]
        edit[rel2] = edit[rel2] + rgb2 * (1 - alpha).numpy()[rel2]
        for k, v in (('rgb_fg', rgb1), ('px_fg', px1), ('py_fg', py1), ('relevant_fg', rel1), ('rgb_bg', rgb2), ('px_bg', px2),
                     ('py_bg', py2), ('relevant_bg', rel2), ('edited_fg', edit1), ('edited_bg', edit2), ('edit', edit)):
            fix[k] = torch.from_numpy(np.ascontiguousarray(v))
        assert 0.2 < rel1.mean() < 0.9 and 0.2 < rel2.mean() < 0.9            # both branches of both layers

        # the masks: rows that never share a cell
        muv_fg, muv_bg = _mask_rows(ev, tex_fg, box_fg, 0.5, 1), _mask_rows(ev, tex_bg, box_bg, -0.5, 2)
        malpha = alpha[:N_MASK]
        masks = [np.zeros((R, R)), np.zeros((R, R))]
        for layer, (uv, shift, box, tex) in enumerate(((muv_fg, 0.5, box_fg, tex_fg), (muv_bg, -0.5, box_bg, tex_bg))):
            _, px, py, rel = _layer(ev, uv, shift, box, tex)
            assert rel.all()
            value = malpha.squeeze()[rel].numpy() if layer == 0 else 1
            touched = np.zeros((R, R), np.int64)
            for fy, fx in ((np.ceil, np.ceil), (np.floor, np.floor), (np.floor, np.ceil), (np.ceil, np.floor)):
                iy, ix = fy(py).astype(np.int64), fx(px).astype(np.int64)
                masks[layer][iy, ix] = np.maximum(masks[layer][iy, ix], value)
                np.add.at(touched, (iy, ix), 1)
            assert touched.max() == 1 and touched.sum() == 4 * N_MASK          # no cell twice: last writer == maximum
        fix.update(mask_uv_fg=muv_fg, mask_uv_bg=muv_bg, mask_alpha=malpha[:, 0].clone(),
                   mask_fg=torch.from_numpy(masks[0]), mask_bg=torch.from_numpy(masks[1]))
    return fix


if __name__ == '__main__':
    fix = generate()
    torch.save(fix, OUT)
    print(OUT, os.path.getsize(OUT), 'bytes; relevant share fg / bg =', float(fix['relevant_fg'].float().mean()),
          float(fix['relevant_bg'].float().mean()))
