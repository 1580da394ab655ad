"""python -m videoswap_amd.extract_points — the DIFT half of extract_semantic_point.py (its __main__, :208-233).

Point tracks come in (`--tracks`: a TAP-like file with `pred_tracks [F, P, 2]` in image pixels and `point_name2id`, from
any tracker or an existing TAP file; a `point_embedding` in it is ignored); the TAP file that `formats.load_tap`, the
product dataset and the reference's frame_point_dataset.py read comes out, with one DIFT embedding per point and, for a
non-human subject, the tracks filtered by DIFT confidence.  CoTracker / OpenPose propagation is out of scope.
"""
import argparse
import os

import torch


def _bool(v):
    if isinstance(v, bool):
        return v
    if v.lower() in ('1', 'true', 'yes', 'y'):
        return True
    if v.lower() in ('0', 'false', 'no', 'n'):
        return False
    raise argparse.ArgumentTypeError(f'expected a boolean, got {v!r}')


def build_parser():
    p = argparse.ArgumentParser(prog='python -m videoswap_amd.extract_points', description=__doc__.split('\n')[0])
    p.add_argument('--frame_dir', required=True, help='frames named by their index (00000.jpg ...)')
    p.add_argument('--tracks', required=True, help='file with pred_tracks [F, P, 2] and point_name2id')
    p.add_argument('--model_id', required=True, help='SD folder (unet/, vae/, text_encoder/, tokenizer/, scheduler/)')
    p.add_argument('--subject_category', required=True, help="prompt = 'photo of a <category>'")
    p.add_argument('--is_human', type=_bool, default=False)
    key = p.add_mutually_exclusive_group()
    key.add_argument('--keyframe_annotation_path', default=None, help='its file stem is the keyframe index')
    key.add_argument('--keyframe', type=int, default=None)
    p.add_argument('--save_path', required=True)
    p.add_argument('--frames_per_call', type=int, default=4, help='frames per UNet call (8 ensemble images each)')
    p.add_argument('--seed', type=int, default=0)
    p.add_argument('--vis_dir', default=None, help='object branch: cosine heat maps of the keyframe points')
    return p


def parse_args(argv=None):
    args = build_parser().parse_args(argv)
    if args.keyframe is None and args.keyframe_annotation_path is not None:
        stem = os.path.splitext(os.path.basename(args.keyframe_annotation_path))[0]
        try:
            args.keyframe = int(stem)
        except ValueError:
            raise SystemExit(f'--keyframe_annotation_path: {stem!r} is not a frame index') from None
    if not args.is_human and args.keyframe is None:
        raise SystemExit('a non-human subject needs --keyframe or --keyframe_annotation_path')
    if args.frames_per_call < 1:
        raise SystemExit('--frames_per_call must be >= 1')
    return args


def run(args, featurizer=None):
    from . import formats
    from .dift import SDFeaturizer, extract_point_embedding
    tap = formats.load_tracks(args.tracks)
    if featurizer is None:
        featurizer = SDFeaturizer(args.model_id, frames_per_call=args.frames_per_call)
    gen = torch.Generator(device=featurizer.device).manual_seed(args.seed)
    out = extract_point_embedding(tap, args.frame_dir, args.keyframe, featurizer, args.subject_category, args.is_human,
                                  frames_per_call=args.frames_per_call, generator=gen,
                                  vis_dir=args.vis_dir)
    formats.save_tap(args.save_path, out['pred_tracks'], out['point_embedding'], out['point_name2id'])
    return out


def main(argv=None):
    run(parse_args(argv))


if __name__ == '__main__':
    main()
