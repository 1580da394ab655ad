"""Records tests/golden/atlas_train_losses.pt: one training step's losses by the reference's own loss code
(videoswap/atlas/loss_utils.py, which needs only torch), on the CPU.

    python tests/golden/make_golden_atlas_train.py

loss_utils.py is IMPORTED from the reference's tree (VIDEOSWAP_REFERENCE, default /root/reference), never copied.  The step
around it (train_atlas.py:135-249 is the body of a loop, not a function) is driven from here: the same calls with the same
arguments.  The networks are the tiny closed-form callables of tests/atlas_train_case.py (elementwise: no matrix product, so
a row's bits do not depend on the rows it is evaluated with), the data_dict its 12 x 8 x 3-frame synthetic one, 40 sampled
pixels, derivative amounts 1 and 3.  Recorded, in fp64 and in fp32, with and without the alpha loss and the global rigidity
losses: every entry of loss_dict, and per network, in the order the reference calls it, each call's output and the
autograd gradient of total_loss with respect to it.
"""
import importlib.util
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
REFERENCE_ROOT = os.environ.get('VIDEOSWAP_REFERENCE', '/root/reference')
OUT = os.path.join(HERE, 'atlas_train_losses.pt')

import atlas_train_case as tc  # noqa: E402


def reference_losses():
    dont = sys.dont_write_bytecode
    sys.dont_write_bytecode = True
    try:
        spec = importlib.util.spec_from_file_location('_ref_loss_utils', os.path.join(REFERENCE_ROOT, 'videoswap', 'atlas', 'loss_utils.py'))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.dont_write_bytecode = dont
    return mod


class Recorded:
    """a callable of the case file behind the interface of a network: casts its input, keeps every output and its gradient"""

    def __init__(self, fn, dtype):
        self.fn, self.dtype, self.outputs = fn, dtype, []

    def __call__(self, x):
        y = self.fn(x.to(self.dtype))
        y.retain_grad()
        self.outputs.append(y)
        return y


def step(lu, data, jif_current, train, with_alpha, with_global, dtype):
    """train_atlas.py:139-249 with the reference's functions"""
    import numpy as np
    nets = {k: Recorded(fn, dtype) for k, fn in tc.TinyNets(dtype).items()}
    FG_UV_Mapping, BG_UV_Mapping, F_Alpha, F_Atlas = (nets[k] for k in ('FG_UV_Mapping', 'BG_UV_Mapping', 'F_Alpha', 'F_Atlas'))
    number_of_frames = data['video_frames'].shape[-1]
    larger_dim = np.maximum(data['video_frames'].shape[0], data['video_frames'].shape[1])
    norm_s = lambda x: x / (larger_dim / 2) - 1  # noqa: E731
    norm_t = lambda x: x / (number_of_frames / 2) - 1  # noqa: E731
    dev, cfg, scale = 'cpu', train['loss_cfg'], train['uv_mapping_scale']
    rgb_current = data['video_frames'][jif_current[1, :], jif_current[0, :], :, jif_current[2, :]].squeeze(1)
    alpha_gt = data['mask_frames'][jif_current[1, :], jif_current[0, :], jif_current[2, :]].squeeze(1).unsqueeze(-1)
    xyt_current = torch.cat([norm_s(jif_current[0, :]), norm_s(jif_current[1, :]), norm_t(jif_current[2, :])], dim=1)
    uv_fg, uv_bg = FG_UV_Mapping(xyt_current), BG_UV_Mapping(xyt_current)
    alpha = 0.5 * (F_Alpha(xyt_current) + 1.0)
    alpha = alpha * 0.99
    alpha = alpha + 0.001
    rgb_output_fg = (F_Atlas(uv_fg * 0.5 + 0.5) + 1.0) * 0.5
    rgb_output_bg = (F_Atlas(uv_bg * 0.5 - 0.5) + 1.0) * 0.5
    rgb_output = rgb_output_fg * alpha + rgb_output_bg * (1.0 - alpha)
    loss_total, loss_dict = 0.0, {}
    loss_dict['gradient_loss'] = lu.get_gradient_loss(data['video_frames_dx'], data['video_frames_dy'], jif_current, FG_UV_Mapping, BG_UV_Mapping,
                                                      F_Atlas, F_Alpha, rgb_output, norm_s, norm_t, device=dev)
    loss_total += cfg['reconstruction_loss']['gradient_loss_weight'] * loss_dict['gradient_loss']
    loss_dict['rgb_loss'] = (torch.norm(rgb_output - rgb_current, dim=1) ** 2).mean()
    loss_total += cfg['reconstruction_loss']['rgb_loss_weight'] * loss_dict['rgb_loss']
    if with_alpha:
        loss_dict['alpha_loss'] = torch.mean(-alpha_gt * torch.log(alpha) - (1 - alpha_gt) * torch.log(1 - alpha))
        loss_total += cfg['reconstruction_loss']['alpha_loss_weight'] * loss_dict['alpha_loss']
    loss_dict['alpha_mean_fg'] = alpha[alpha > 0.5].mean()
    loss_dict['alpha_mean_bg'] = alpha[alpha < 0.5].mean()
    loss_dict['sparsity_loss'] = (torch.norm(rgb_output_fg * (1.0 - alpha), dim=1) ** 2).mean()
    loss_total += cfg['sparsity_loss']['sparsity_loss_weight'] * loss_dict['sparsity_loss']
    for key, amount, weights in (('rigidity_loss', train['derivative_amount'], ('rigidity_loss_weight', 'rigidity_loss_weight')),
                                 ('global_rigidity_loss', train['global_derivative_amount'],
                                  ('global_rigidity_fg_loss_weight', 'global_rigidity_bg_loss_weight')))[:2 if with_global else 1]:
        for layer, net, uv, weight in (('fg', FG_UV_Mapping, uv_fg, weights[0]), ('bg', BG_UV_Mapping, uv_bg, weights[1])):
            loss_dict[f'{key}_{layer}'] = lu.get_rigidity_loss(jif_current, amount, larger_dim, net, uv, scale, norm_s, norm_t, device=dev)
            loss_total += cfg['rigidity_loss'][weight] * loss_dict[f'{key}_{layer}']
    for layer, net, uv, weight in (('fg', FG_UV_Mapping, uv_fg, alpha), ('bg', BG_UV_Mapping, uv_bg, 1 - alpha)):
        loss_dict[f'flow_loss_{layer}'] = lu.get_optical_flow_loss(
            jif_current, uv, data['optical_flows_reverse'], data['optical_flows_reverse_mask'], larger_dim, net, data['optical_flows'],
            data['optical_flows_mask'], scale, norm_s, norm_t, device=dev, use_alpha=True, alpha=weight)
        loss_total += cfg['flow_loss']['flow_loss_weight'] * loss_dict[f'flow_loss_{layer}']
    loss_dict['flow_alpha_loss'] = lu.get_optical_flow_alpha_loss(
        F_Alpha, jif_current, alpha, data['optical_flows_reverse'], data['optical_flows_reverse_mask'], norm_s, norm_t, data['optical_flows'],
        data['optical_flows_mask'], device=dev)
    loss_total += cfg['flow_loss']['alpha_flow_loss_weight'] * loss_dict['flow_alpha_loss']
    loss_dict['total_loss'] = loss_total
    loss_total.backward()
    return {'loss_dict': {k: v.detach() for k, v in loss_dict.items()},
            'outputs': {k: [y.detach() for y in n.outputs] for k, n in nets.items()},
            'grads': {k: [y.grad for y in n.outputs] for k, n in nets.items()}}


def reference_available():
    return os.path.isfile(os.path.join(REFERENCE_ROOT, 'videoswap', 'atlas', 'loss_utils.py'))


def generate(data=None, idx=None):
    """the fixture; `data` / `idx`: inputs to use instead of fresh ones (a recorded fixture's, for a re-run on another machine)"""
    lu = reference_losses()
    c = tc.GOLDEN_CASE
    data = tc.synthetic_data(c['W'], c['H'], c['T'], c['seed']) if data is None else data
    idx = tc.sample(data, c['N'], c['seed'], corners=True) if idx is None else idx
    jif = tc.jif_of(idx, c['H'], c['W'])
    train = dict(tc.TRAIN, derivative_amount=c['derivative_amount'], global_derivative_amount=c['global_derivative_amount'])
    runs = {}
    for flags in ((True, True), (False, False)):
        for dtype, tag in ((torch.float64, 'fp64'), (torch.float32, 'fp32')):
            runs[(flags, tag)] = step(lu, data, jif, train, *flags, dtype)
    return {'case': c, 'data': data, 'idx': idx, 'train': train, 'runs': runs}


def main():
    fix = generate()
    torch.save(fix, OUT)
    print(f'wrote {OUT}: {os.path.getsize(OUT)} bytes')
    for (flags, tag), r in fix['runs'].items():
        print(flags, tag, {k: float(v) for k, v in r['loss_dict'].items()})


if __name__ == '__main__':
    main()
