"""The fused coordinate MLP (csrc/atlas.hip) and the atlas point propagation on the MI355X.

Kernel parity: the yardstick is an fp64 PyTorch evaluation of the same network on the CPU.  No tolerance is fixed in
advance: fp32 PyTorch (an F.linear chain on the CPU) is measured against the same fp64 evaluation on the same inputs, and
the kernel's max-abs error must be at most 4 x that (the margin covers another summation order over K <= 286).  Both
errors are printed and collected in profiles/atlas_parity.json (written when VSX_WRITE_PROFILES=1).

Propagation: on the kernel against the reference's fixture (atlas_case.compare_tracks), and at the real widths (hidden
256, T = 72, P = 16) against the same host code on the CPU stand-in.
"""
import json
import os

import pytest
import torch

import atlas_case
from atlas_case import build_models, compare_tracks, counted, ref_forward, standin, write_case
from util import ROOT

pytestmark = pytest.mark.gpu

FG = dict(input_dim=3, output_dim=2, hidden_dim=256, pe_type='none', pe_dim=4, mlp_layers=6, skip_layers=[])
INV = dict(FG, output_dim=3)
ALPHA = dict(input_dim=3, output_dim=1, hidden_dim=256, pe_type='encoding', pe_dim=5, mlp_layers=8, skip_layers=[])
SKIP = dict(input_dim=2, output_dim=3, hidden_dim=256, pe_type='none', pe_dim=4, mlp_layers=8, skip_layers=[4, 7])
# (name, constructor arguments, N): the row sweep (tile edges, one row, every pixel of a 768 x 448 frame) on ONE network
CASES = [('fg', FG, n) for n in (1, 63, 64, 65, 1000, 344064)] + [
    ('inverse', INV, 1000), ('alpha', ALPHA, 1000), ('skip_4_7', SKIP, 1000),
    ('hidden64', dict(FG, hidden_dim=64), 1000), ('hidden32', dict(ALPHA, hidden_dim=32), 1000),
    ('no_tanh', dict(INV, use_tanh=False, hidden_dim=128, mlp_layers=2), 65)]
_parity = []


def _network(kw, scale, seed):
    from videoswap_amd.atlas import CoordMLP
    torch.manual_seed(seed)
    m = CoordMLP(**kw)                                   # nn.Linear default initialisation
    with torch.no_grad():
        for q in m.parameters():
            q.mul_(scale)
    return m


# weights at the nn.Linear default initialisation and at twice that scale; the 344 064-row case runs once
RUNS = [c + (s,) for c in CASES for s in (1.0, 2.0) if not (c[2] > 100000 and s != 1.0)]


@pytest.mark.parametrize('name,kw,N,scale', RUNS, ids=[f'{c[0]}-{c[2]}-x{c[3]:g}' for c in RUNS])
def test_kernel_against_fp64(name, kw, N, scale):
    m = _network(kw, scale, seed=N % 1000 + len(name))
    g = torch.Generator().manual_seed(N)
    x = torch.rand(N, kw['input_dim'], generator=g) * 2 - 1
    with torch.no_grad():
        y64 = ref_forward(m, x, torch.float64)
        y32 = ref_forward(m, x, torch.float32)
        got = m.cuda()(x.cuda()).cpu()
    assert got.shape == y64.shape and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
    err_torch = float((y32.double() - y64).abs().max())
    err_kernel = float((got.double() - y64).abs().max())
    print(f'coord_mlp {name} N={N} scale={scale}: fp32 torch vs fp64 {err_torch:.3e}, kernel vs fp64 {err_kernel:.3e}, '
          f'max |y| {float(y64.abs().max()):.3f}')
    _parity.append({'case': name, 'N': N, 'weight_scale': scale, 'err_fp32_torch': err_torch, 'err_kernel': err_kernel,
                    'bound': 4 * err_torch})
    assert err_kernel <= 4 * err_torch, (err_kernel, err_torch)


def test_parity_figures_recorded():
    """runs after the parity cases (file order): all of them left a figure; VSX_WRITE_PROFILES=1 writes the profile"""
    assert len(_parity) == len(RUNS)
    if os.environ.get('VSX_WRITE_PROFILES') == '1':
        out = os.environ.get('VSX_PROFILE_DIR', os.path.join(ROOT, 'profiles'))
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, 'atlas_parity.json'), 'w') as f:
            json.dump({'device': torch.cuda.get_device_name(0), 'rule': 'err_kernel <= 4 * err_fp32_torch (max abs, vs fp64)',
                       'cases': _parity}, f, indent=1)


def test_unsupported_sizes_come_back_from_the_entry_point():
    from videoswap_amd import ops
    x, w = torch.zeros(4, 3, device='cuda'), torch.zeros(64, device='cuda')
    for kw, word in ((dict(pe_type='hash_encoding'), 'hash_encoding'), (dict(mlp_type='tcnn'), 'tcnn'),
                     (dict(hidden_dim=48), 'hidden_dim'), (dict(hidden_dim=512), 'hidden_dim'), (dict(mlp_layers=9), 'mlp_layers'),
                     (dict(mlp_layers=1), 'mlp_layers'), (dict(output_dim=4), 'output_dim'), (dict(skip_layers=[0]), 'skip_layers'),
                     (dict(pe_type='encoding', pe_dim=11), 'pe_dim')):
        args = dict(input_dim=3, output_dim=2, hidden_dim=64, mlp_layers=4)
        args.update(kw)
        with pytest.raises(NotImplementedError, match=word):
            ops.coord_mlp(x, w, **args)
    from videoswap_amd._lib import VsxError
    with pytest.raises(VsxError, match='packed'):                            # a buffer of the wrong size is refused, not read
        ops.coord_mlp(x, w, 3, 2, 64, 4)


def _run_propagation(fix, tmp, device, keep=None):
    from videoswap_amd import atlas
    models = build_models(fix, device)
    os.makedirs(str(tmp), exist_ok=True)
    src, tap, tgt = write_case(str(tmp), fix, keep)
    ds = fix['config']['datasets']
    return atlas.propagate_point_sequence(src, tap, tgt, *models, larger_dim=max(ds['res_x'], ds['res_y']),
                                          number_of_frames=fix['number_of_frames'], return_details=True)


def test_propagation_on_the_kernel_matches_the_reference(tmp_path):
    fix = torch.load(atlas_case.FIXTURE, map_location='cpu', weights_only=True)
    with counted() as box:
        out, details = _run_propagation(fix, tmp_path, 'cuda')
    figures = compare_tracks(fix, out, details)
    print('propagation on the kernel vs reference:', figures)
    assert box['calls'] == 3
    assert torch.equal(out['point_embedding'], fix['tap']['point_embedding'])


def _wide_case(P, T, seed=3, alpha_shift=0.0):
    """hidden 256 networks of the swan config (weights at 2 x the default initialisation), P dragged points, T frames;
    `alpha_shift` is added to the last bias of F_Alpha"""
    from videoswap_amd.atlas import MODEL_NAMES
    specs = dict(zip(MODEL_NAMES, (FG, INV, ALPHA)))
    g = torch.Generator().manual_seed(seed)
    names = [f'p{i}' for i in range(P)]
    source = {n: [float(torch.randint(40, 408, (1,), generator=g)), float(torch.randint(40, 728, (1,), generator=g))] for n in names}
    target = {n: [v[0] + float(torch.randint(-30, 30, (1,), generator=g)), v[1] + float(torch.randint(-30, 30, (1,), generator=g))]
              for n, v in source.items()}
    sd = {}
    for i, (name, kw) in enumerate(specs.items()):
        m = _network(kw, 2.0, seed=50 + i)
        if name == 'F_Alpha':
            with torch.no_grad():
                m.hidden[-1].bias.add_(alpha_shift)
        sd[name] = m.state_dict()
    return {'config': {'models': specs, 'datasets': {'res_x': 768, 'res_y': 448, 'max_frames': T}}, 'state_dicts': sd,
            'source_points': source, 'target_points': target, 'keyframe': 7, 'number_of_frames': T,
            'tap': {'pred_tracks': torch.rand(T + 2, P, 2, generator=g) * 400, 'point_name2id': {n: i for i, n in enumerate(names)},
                    'point_embedding': torch.randn(P, 8, generator=g)}}


def test_propagation_at_real_widths_matches_the_host_code_on_the_stand_in(tmp_path):
    """the stand-in's result takes the place of the reference's in the same comparison rule.  F_Alpha's last bias is set
    from a first stand-in run so that the median alpha is 0.5: both visibility branches occur, about half each."""
    with standin():
        first = _run_propagation(_wide_case(P=16, T=72), tmp_path / 'first', 'cpu')[1]['alpha']
    shift = -float(torch.atanh((2 * first - 1).double().clamp(-0.999999, 0.999999)).median())
    case = _wide_case(P=16, T=72, alpha_shift=shift)
    with standin():
        ref_out, ref_details = _run_propagation(case, tmp_path / 'cpu', 'cpu')
    case['pred_tracks'] = ref_out['pred_tracks']
    visible = ref_details['alpha'] > 0.5
    case['alpha'] = ref_details['alpha']
    case['pixels'] = torch.where(visible.unsqueeze(-1), ref_details['pixels'], torch.full_like(ref_details['pixels'], float('nan')))
    with counted() as box:
        out, details = _run_propagation(case, tmp_path / 'gpu', 'cuda')
    figures = compare_tracks(case, out, details)
    print('propagation at hidden 256, P 16, T 72, kernel vs stand-in:', figures, 'visible share', float(visible.float().mean()))
    assert box['calls'] == 3 and 0.25 <= float(visible.float().mean()) <= 0.75


def test_launch_count_does_not_depend_on_points_or_frames(tmp_path):
    counts = []
    for P, T in ((1, 8), (16, 72)):
        case = _wide_case(P, T)
        with counted() as box:
            _run_propagation(case, tmp_path / f'{P}_{T}', 'cuda')
        counts.append(box['calls'])
    assert counts == [3, 3]
