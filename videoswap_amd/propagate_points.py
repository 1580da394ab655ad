"""python -m videoswap_amd.propagate_points — propagate_point_displacement.py (its __main__, :149-180) on the GPU.

A trained atlas (its YAML and its checkpoint), the keyframe's source points, the source TAP file and the dragged target
points come in; `TAP_<target stem>.pth` comes out beside the target file (or at `--save_path`), in the layout
`formats.load_tap` and the reference's frame_point_dataset.py read.  No frame, mask or flow is read: the number of frames
is min(datasets.max_frames, files in datasets.frame_path) or `--num_frames`; the visualisation of the reference is not
produced.
"""
import argparse
import os

from .atlas_cli import add_atlas_arguments, add_frame_arguments, open_atlas


def build_parser():
    p = argparse.ArgumentParser(prog='python -m videoswap_amd.propagate_points', description=__doc__.split('\n')[0])
    add_atlas_arguments(p, 'FG_UV_Mapping, FG_UV_Mapping_Inverse, F_Alpha')
    p.add_argument('--source_point_path', required=True, help='<keyframe index>.json: {name: [y, x]}')
    p.add_argument('--source_tap_path', required=True)
    p.add_argument('--target_point_path', required=True, help='{name: [y, x]} of the dragged points')
    add_frame_arguments(p, frames=False)
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
    models, T, W, H, _, device = open_atlas(args, device, atlas.MODEL_NAMES, args.num_frames)
    tap = atlas.propagate_point_sequence(args.source_point_path, args.source_tap_path, args.target_point_path,
                                         *(models[k] for k in atlas.MODEL_NAMES), larger_dim=max(W, H), number_of_frames=T,
                                         device=device)
    formats.save_tap(args.save_path, tap['pred_tracks'], tap['point_embedding'], tap['point_name2id'])
    print(f'save to {args.save_path}')
    return tap


def main(argv=None):
    run(parse_args(argv))


if __name__ == '__main__':
    main()
