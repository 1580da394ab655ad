"""python -m videoswap_amd.refit_atlas — refit a trained atlas's texture to its frames on the GPU.

A trained atlas (its YAML and its checkpoint), the video frames (`--frame_dir`, sorted by name; resized to res_x x res_y when
they differ, as render_atlas reads them) and the foreground masks (`--mask_dir`, as load_input_data reads them) come in;
`--iters` steps of the reconstruction half of the training step (atlas.fit_reconstruction: the rgb, alpha and sparsity
losses of train_atlas.py) are run on the networks named by `--train`, and `--save_path` receives a
checkpoint that the other tools load: every entry of the input checkpoint, the trained networks replaced.  By default only
F_Atlas is trained and the mapping networks stay frozen, so the parametrisation stays valid for point propagation and for
textures edited earlier.  The gradient, rigidity and flow losses of train_atlas.py are not used here
(videoswap_amd.train_atlas runs them): with the mapping networks in `--train` nothing keeps the mappings rigid.
"""
import argparse
import os

import torch

from .atlas_cli import add_atlas_arguments, add_frame_arguments, open_atlas


def build_parser():
    p = argparse.ArgumentParser(prog='python -m videoswap_amd.refit_atlas', description=__doc__.split('\n')[0])
    add_atlas_arguments(p, 'the five networks')
    p.add_argument('--frame_dir', required=True, help='the video frames')
    p.add_argument('--mask_dir', required=True, help='the foreground masks, in the same order')
    p.add_argument('--iters', type=int, required=True)
    p.add_argument('--save_path', required=True, help='the checkpoint to write')
    p.add_argument('--train', default='F_Atlas', help='comma-separated networks to train (default: F_Atlas)')
    p.add_argument('--batch', type=int, default=10000, help='pixels per step (datasets.sample_batch_size)')
    p.add_argument('--lr', type=float, default=1e-4)
    p.add_argument('--seed', type=int, default=None, help='seeds the sampling')
    add_frame_arguments(p, frames=False)
    return p


def parse_args(argv=None):
    args = build_parser().parse_args(argv)
    args.train = tuple(v.strip() for v in args.train.split(',') if v.strip())
    return args


def run(args, device=None):
    from . import atlas, atlas_fit, formats
    from .render_atlas import IMAGE_EXT, _read_images
    unknown = [k for k in args.train if k not in atlas_fit.NETWORKS]
    if unknown or not args.train:
        raise SystemExit(f'--train: {args.train} must name some of {atlas_fit.NETWORKS}')
    num_frames = args.num_frames
    if num_frames is None:
        num_frames = len([n for n in os.listdir(args.frame_dir) if n.lower().endswith(IMAGE_EXT)])
    models, T, W, H, _, _ = open_atlas(args, device, atlas.RENDER_MODEL_NAMES, num_frames)
    video = _read_images(args.frame_dir, list(range(T)), (W, H), 'RGB').permute(1, 2, 3, 0).contiguous()    # [H, W, 3, T]
    masks = atlas.load_mask_frames(args.mask_dir, W, H, T)
    config = atlas.load_atlas_config(args.atlas_config_path)
    loss_cfg = (config.get('train') or {}).get('loss_cfg')
    if args.seed is not None:
        torch.manual_seed(args.seed)
    history = atlas.fit_reconstruction(models, video, masks, args.iters, batch=args.batch, lr=args.lr, train=args.train,
                                       loss_cfg=loss_cfg)
    ckpt = dict(formats._load(args.atlas_model_path))
    for k in args.train:
        ckpt[k] = {name: v.detach().cpu() for name, v in models[k].state_dict().items()}
    os.makedirs(os.path.dirname(os.path.abspath(args.save_path)), exist_ok=True)
    torch.save(ckpt, args.save_path)
    if history:
        print(f'{len(history)} steps on {", ".join(args.train)}: loss {history[0]:.6g} -> {history[-1]:.6g}')
    print(f'save to {args.save_path}')
    return history


def main(argv=None):
    run(parse_args(argv))


if __name__ == '__main__':
    main()
