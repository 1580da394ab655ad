"""python -m videoswap_amd.propagate_points — propagate_point_displacement.py (its __main__, :149-180) on the GPU.

A trained atlas (its YAML and its checkpoint), the keyframe's source points, the source TAP file and the dragged target
points come in; `TAP_<target stem>.pth` comes out beside the target file (or at `--save_path`), in the layout
`formats.load_tap` and the reference's frame_point_dataset.py read.  No frame, mask or flow is read: the number of frames
is min(datasets.max_frames, files in datasets.frame_path) or `--num_frames`; the visualisation of the reference is not
produced.
"""
import argparse
import os

import torch


def build_parser():
    p = argparse.ArgumentParser(prog='python -m videoswap_amd.propagate_points', description=__doc__.split('\n')[0])
    p.add_argument('--atlas_config_path', required=True, help="the atlas's training YAML (models.*, datasets.*)")
    p.add_argument('--atlas_model_path', required=True, help='checkpoint with FG_UV_Mapping, FG_UV_Mapping_Inverse, F_Alpha')
    p.add_argument('--source_point_path', required=True, help='<keyframe index>.json: {name: [y, x]}')
    p.add_argument('--source_tap_path', required=True)
    p.add_argument('--target_point_path', required=True, help='{name: [y, x]} of the dragged points')
    p.add_argument('--num_frames', type=int, default=None, help='stands in for the file count of datasets.frame_path')
    p.add_argument('--save_path', default=None, help='default: TAP_<target stem>.pth beside the target file')
    return p


def parse_args(argv=None):
    args = build_parser().parse_args(argv)
    stem = os.path.splitext(os.path.basename(args.source_point_path))[0]
    try:
        int(stem)
    except ValueError:
        raise SystemExit(f'--source_point_path: {stem!r} is not a frame index') from None
    if args.save_path is None:
        suffix = os.path.splitext(os.path.basename(args.target_point_path))[0]
        args.save_path = os.path.join(os.path.dirname(args.target_point_path), f'TAP_{suffix}.pth')
    return args


def run(args, device=None):
    from . import atlas, formats
    if device is None:
        device = torch.device('cuda')         # the networks run on the HIP kernel only
    config = atlas.load_atlas_config(args.atlas_config_path)
    models = atlas.load_atlas_models(config, args.atlas_model_path, device=device)
    T = atlas.number_of_frames(config, args.num_frames)
    larger_dim = max(int(config['datasets']['res_x']), int(config['datasets']['res_y']))
    tap = atlas.propagate_point_sequence(args.source_point_path, args.source_tap_path, args.target_point_path, *models,
                                         larger_dim=larger_dim, number_of_frames=T, device=device)
    formats.save_tap(args.save_path, tap['pred_tracks'], tap['point_embedding'], tap['point_name2id'])
    print(f'save to {args.save_path}')
    return tap


def main(argv=None):
    run(parse_args(argv))


if __name__ == '__main__':
    main()
