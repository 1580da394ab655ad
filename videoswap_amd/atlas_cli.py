"""What the atlas commands (propagate_points, render_atlas, edit_atlas) share: the arguments that name an atlas, the
`--frames` list, and the opening of a run: config, networks, frame count and size."""
import torch


def add_atlas_arguments(p, networks):
    p.add_argument('--atlas_config_path', required=True, help="the atlas's training YAML (models.*, datasets.*)")
    p.add_argument('--atlas_model_path', required=True, help=f'checkpoint with {networks}')


def add_frame_arguments(p, frames=True):
    p.add_argument('--num_frames', type=int, default=None, help='stands in for the file count of datasets.frame_path')
    if frames:
        p.add_argument('--frames', default=None, help='comma-separated frame indices to render (default: all)')


def parse_frames(args):
    """`--frames` as a list of ints (None stays None)"""
    if args.frames is not None:
        try:
            args.frames = [int(v) for v in args.frames.split(',') if v.strip() != '']
        except ValueError:
            raise SystemExit(f'--frames: {args.frames!r} is not a comma-separated list of frame indices') from None
    return args


def open_atlas(args, device, names, num_frames):
    """-> (models: `names` of the checkpoint on `device`, default the GPU: the networks run on the HIP kernels only;
    T, where `num_frames` stands in for the file count; W; H; frames: `--frames`, default all; device)"""
    from . import atlas
    device = torch.device('cuda') if device is None else device
    config = atlas.load_atlas_config(args.atlas_config_path)
    models = atlas.load_atlas_models(config, args.atlas_model_path, device=device, names=names)
    T = atlas.number_of_frames(config, num_frames)
    frames = getattr(args, 'frames', None)
    return (models, T, int(config['datasets']['res_x']), int(config['datasets']['res_y']),
            list(range(T)) if frames is None else frames, device)
