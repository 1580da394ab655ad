"""python -m videoswap_amd.render_atlas — look at a trained atlas: evaluate_model (videoswap/atlas/evaluate.py:202-591) on the GPU.

A trained atlas (its YAML and its checkpoint) comes in; `--save_dir` receives
  reconstruction/<frame>.png   the video as the five networks reproduce it,
  alpha/<frame>.png            the foreground matte,
  texture_orig1.png            the foreground atlas, [0, 1]^2 at 1000 x 1000,
  texture_orig2.png            the background atlas over the box its mapping reaches, at 1000 x 1000,
  summary.json                 the two mapping boxes, the launch count and, with `--frame_dir`, the PSNR per frame and its mean.
`--frame_dir` holds the video frames (sorted by name; resized to res_x x res_y when they differ), `--mask_dir` the
foreground masks in the same order (the foreground box of the summary then covers masked pixels only, as the reference's).
The edited reconstructions and the checkerboard composites are `python -m videoswap_amd.edit_atlas`'s (it takes this
directory as `--render_dir`); the annotated texture, the loss videos and the mp4 writers of the reference are not produced.
"""
import argparse
import json
import os

import numpy as np
import torch
from PIL import Image

from .atlas_cli import add_atlas_arguments, add_frame_arguments, open_atlas, parse_frames

IMAGE_EXT = ('.png', '.jpg', '.jpeg', '.bmp')


def build_parser():
    p = argparse.ArgumentParser(prog='python -m videoswap_amd.render_atlas', description=__doc__.split('\n')[0])
    add_atlas_arguments(p, 'the five networks')
    p.add_argument('--save_dir', required=True)
    p.add_argument('--frame_dir', default=None, help='video frames to compute the PSNR against')
    p.add_argument('--mask_dir', default=None, help='foreground masks (for the foreground box)')
    add_frame_arguments(p)
    p.add_argument('--texture_resolution', type=int, default=1000)
    return p


def parse_args(argv=None):
    return parse_frames(build_parser().parse_args(argv))


def _read_images(directory, indices, size, mode):
    """the files of `directory` (sorted) at `indices` -> float32 [len, H, W, C or nothing] in [0, 1]"""
    names = sorted(n for n in os.listdir(directory) if n.lower().endswith(IMAGE_EXT))
    if indices and max(indices) >= len(names):
        raise SystemExit(f'{directory}: {len(names)} images, frame {max(indices)} asked for')
    out = []
    for i in indices:
        img = Image.open(os.path.join(directory, names[i])).convert(mode)
        if img.size != size:
            img = img.resize(size, Image.BILINEAR)
        out.append(np.asarray(img, dtype=np.float32) / 255.0)
    return torch.from_numpy(np.stack(out)) if out else torch.zeros(0)


def _save_image(array01, path):
    """[H, W] or [H, W, 3] in [0, 1] -> 8-bit PNG"""
    Image.fromarray((array01.clamp(0, 1) * 255).round().to(torch.uint8).cpu().numpy()).save(path)


def write_frames(save_dir, sub, images, frames):
    """images[k] -> <save_dir>/<sub>/<frames[k]>.png"""
    os.makedirs(os.path.join(save_dir, sub), exist_ok=True)
    for k, f in enumerate(frames):
        _save_image(images[k], os.path.join(save_dir, sub, f'{f:05d}.png'))


def run(args, device=None):
    from . import atlas
    num_frames = args.num_frames
    if num_frames is None and args.frame_dir:
        num_frames = len([n for n in os.listdir(args.frame_dir) if n.lower().endswith(IMAGE_EXT)])
    models, T, W, H, frames, _ = open_atlas(args, device, atlas.RENDER_MODEL_NAMES, num_frames)

    out = atlas.render_atlas(models, W, H, T, frames=frames)
    for sub in ('reconstruction', 'alpha'):
        write_frames(args.save_dir, sub, out[sub], frames)
    launches = out['launches']

    # the two boxes of evaluate_model:217-220 (over ALL frames of the atlas, as there)
    masks = None
    if args.mask_dir:
        masks = _read_images(args.mask_dir, list(range(T)), (W, H), 'L') > 0.5
    FG, BG, F_Alpha, F_Atlas = (models[k] for k in ('FG_UV_Mapping', 'BG_UV_Mapping', 'F_Alpha', 'F_Atlas'))
    bg = atlas.mapping_area(BG, F_Alpha, W, H, T, -0.5, masks=None, invert_alpha=True)
    fg = atlas.mapping_area(FG, F_Alpha, W, H, T, 0.5, masks=masks, invert_alpha=False, alpha_thresh=0.95)
    n = int(args.texture_resolution)
    _save_image(atlas.atlas_texture(F_Atlas, n, 0, 1, 0, 1), os.path.join(args.save_dir, 'texture_orig1.png'))
    maxx2, minx2, maxy2, miny2, edge2 = bg
    _save_image(atlas.atlas_texture(F_Atlas, n, minx2, minx2 + edge2, miny2, miny2 + edge2),
                os.path.join(args.save_dir, 'texture_orig2.png'))

    keys = ('maxx', 'minx', 'maxy', 'miny', 'edge_size')
    summary = {'config': os.path.abspath(args.atlas_config_path), 'checkpoint': os.path.abspath(args.atlas_model_path),
               'res_x': W, 'res_y': H, 'number_of_frames': T, 'frames': frames, 'render_launches': launches,
               'foreground_box': dict(zip(keys, fg)), 'background_box': dict(zip(keys, bg)),
               'foreground_box_uses_masks': masks is not None}
    if args.frame_dir:
        video = _read_images(args.frame_dir, frames, (W, H), 'RGB')
        per_frame, mean = atlas.atlas_psnr(out['reconstruction'], video)
        summary['psnr_per_frame'] = {f'{f:05d}': float(v) for f, v in zip(frames, per_frame)}
        summary['psnr_mean'] = mean
    with open(os.path.join(args.save_dir, 'summary.json'), 'w') as fw:
        json.dump(summary, fw, indent=1)
    print(f'save to {args.save_dir}')
    return summary


def main(argv=None):
    run(parse_args(argv))


if __name__ == '__main__':
    main()
