"""python -m videoswap_amd.edit_atlas — edit a video through its atlas: the second half of evaluate_model (videoswap/atlas/evaluate.py:344-444) on the GPU.

`python -m videoswap_amd.render_atlas` exports the two atlas textures (`texture_orig1.png`: the foreground over
[0, 1]^2, `texture_orig2.png`: the background over the box its mapping reaches).  Paint on them, hand them back with
`--edit_fg` / `--edit_bg`, and `--save_dir` receives
  edit/<frame>.png             the video with the paint following the object,
  edited_fg/<frame>.png        the foreground layer alone (times its alpha),
  edited_bg/<frame>.png        the background layer alone,
  checkerboard_fg/, checkerboard_bg/   with `--checkerboard`: a checkerboard laid over each atlas, seen through the mappings,
  texture_edit1.png, texture_edit2.png with `--write_masks`: each texture times its "was this texel ever used" mask,
  summary.json                 the boxes, the launch count and the share of pixels each layer reaches.
`--render_dir` is the render_atlas output directory: the boxes come from its summary.json, the texture resolution from
the PNG size, and without `--edit_fg` / `--edit_bg` its own textures are used (an identity edit: `edit` then repeats
`reconstruction` up to the 8-bit texture).  An RGB file REPLACES the texture; an RGBA file is laid OVER the colour the
texture network gives (alpha 0 keeps the atlas).
PNGs are written by rounding and clamping, as render_atlas writes them; the reference's truncating astype(uint8), its
mp4 writers, the cv2 text pattern of `edited_tex`, the griddata alpha masks and the loss videos are not reproduced.
"""
import argparse
import json
import os

import numpy as np
import torch
from PIL import Image

from .atlas_cli import add_atlas_arguments, add_frame_arguments, open_atlas, parse_frames
from .render_atlas import IMAGE_EXT, _save_image, write_frames


def build_parser():
    p = argparse.ArgumentParser(prog='python -m videoswap_amd.edit_atlas', description=__doc__.split('\n')[0])
    add_atlas_arguments(p, 'the five networks')
    p.add_argument('--save_dir', required=True)
    p.add_argument('--render_dir', required=True, help='output directory of videoswap_amd.render_atlas (summary.json, texture_orig*.png)')
    p.add_argument('--edit_fg', default=None, help='edited foreground texture (RGB replaces, RGBA overlays); default: texture_orig1.png')
    p.add_argument('--edit_bg', default=None, help='edited background texture (RGB replaces, RGBA overlays); default: texture_orig2.png')
    add_frame_arguments(p)
    p.add_argument('--checkerboard', action='store_true', help='also write the checkerboard composites')
    p.add_argument('--write_masks', action='store_true', help='also write texture_edit1.png / texture_edit2.png')
    return p


def parse_args(argv=None):
    return parse_frames(build_parser().parse_args(argv))


def _read_texture(path):
    """PNG -> float32 [R, R, 3] (any mode without alpha) or [R, R, 4] (a mode with alpha) in [0, 1]"""
    if not path.lower().endswith(IMAGE_EXT) or not os.path.isfile(path):
        raise SystemExit(f'{path}: not an image file')
    img = Image.open(path)
    img = img.convert('RGBA' if 'A' in img.getbands() else 'RGB')
    if img.size[0] != img.size[1]:
        raise SystemExit(f'{path}: {img.size[0]} x {img.size[1]}, a texture must be square')
    return torch.from_numpy(np.asarray(img, dtype=np.float32) / 255.0)


def run(args, device=None):
    from . import atlas
    with open(os.path.join(args.render_dir, 'summary.json')) as fr:
        rendered = json.load(fr)
    num_frames = args.num_frames if args.num_frames is not None else rendered.get('number_of_frames')
    models, T, W, H, frames, device = open_atlas(args, device, atlas.RENDER_MODEL_NAMES, num_frames)

    tex_fg = _read_texture(args.edit_fg or os.path.join(args.render_dir, 'texture_orig1.png')).to(device)
    tex_bg = _read_texture(args.edit_bg or os.path.join(args.render_dir, 'texture_orig2.png')).to(device)
    area_bg = rendered['background_box']
    box_fg = atlas.texture_box(0, 0, 1, tex_fg.shape[0])                                       # evaluate_model:214-216, 222
    box_bg = atlas.texture_box(area_bg['minx'], area_bg['miny'], area_bg['edge_size'], tex_bg.shape[0])

    out = atlas.edit_atlas(models, W, H, T, tex_fg, box_fg, tex_bg, box_bg, frames=frames, want_masks=args.write_masks)
    launches = out['launches']
    for sub in ('edit', 'edited_fg', 'edited_bg'):
        write_frames(args.save_dir, sub, out[sub], frames)
    if args.write_masks:                                                                       # evaluate_model:436-444
        _save_image(out['mask_fg'].unsqueeze(-1) * tex_fg[..., :3], os.path.join(args.save_dir, 'texture_edit1.png'))
        _save_image(out['mask_bg'].unsqueeze(-1) * tex_bg[..., :3], os.path.join(args.save_dir, 'texture_edit2.png'))
    if args.checkerboard:
        area_fg = rendered['foreground_box']
        boards = atlas.checkerboard_videos(models, W, H, T, (area_fg['minx'], area_fg['miny'], area_fg['edge_size']),
                                           (area_bg['minx'], area_bg['miny'], area_bg['edge_size']), frames=frames)
        launches += boards['launches']
        for sub in ('checkerboard_fg', 'checkerboard_bg'):
            write_frames(args.save_dir, sub, boards[sub], frames)

    rel = out['relevant']
    n = max(rel.numel(), 1)
    summary = {'config': os.path.abspath(args.atlas_config_path), 'checkpoint': os.path.abspath(args.atlas_model_path),
               'render_dir': os.path.abspath(args.render_dir), 'res_x': W, 'res_y': H, 'number_of_frames': T, 'frames': frames,
               'edit_fg': args.edit_fg, 'edit_bg': args.edit_bg,
               'texture_fg': {'resolution': int(tex_fg.shape[0]), 'channels': int(tex_fg.shape[2]), 'box': list(box_fg)},
               'texture_bg': {'resolution': int(tex_bg.shape[0]), 'channels': int(tex_bg.shape[2]), 'box': list(box_bg)},
               'edit_launches': out['launches'], 'launches': launches,
               'relevant_share_fg': float(((rel & 1) != 0).sum()) / n, 'relevant_share_bg': float(((rel & 2) != 0).sum()) / n}
    with open(os.path.join(args.save_dir, 'summary.json'), 'w') as fw:
        json.dump(summary, fw, indent=1)
    print(f'save to {args.save_dir}')
    return summary


def main(argv=None):
    run(parse_args(argv))


if __name__ == '__main__':
    main()
