"""python -m videoswap_amd.fit_inverse — give a trained atlas its inverse mapping network (train_atlas.py:255-266) on the GPU.

An atlas checkpoint without `FG_UV_Mapping_Inverse`, or with a poor one, and its YAML come in; the checkpoint with a fitted
`FG_UV_Mapping_Inverse` comes out at `--save_path` (the keys of train_atlas.py:311-318; every other entry is copied
through), so that `python -m videoswap_amd.propagate_points` can use the atlas.  Foreground pixels are those of the masks in
`--mask_dir` (read as load_input_data reads them) or, without masks, those where F_Alpha says foreground.  When the YAML has
no `models.FG_UV_Mapping_Inverse`, the network is `models.FG_UV_Mapping` with `output_dim: 3`, as in the reference's
`*_inv_*` configs; the YAML with the entry actually used is written beside the checkpoint (`<save_path stem>.yml`), and
propagate_points accepts that pair.  An inverse already in the checkpoint is the starting point when it fits the spec.
"""
import argparse
import copy
import os

import torch

from .atlas_cli import add_atlas_arguments, add_frame_arguments


def build_parser():
    p = argparse.ArgumentParser(prog='python -m videoswap_amd.fit_inverse', description=__doc__.split('\n')[0])
    add_atlas_arguments(p, 'FG_UV_Mapping and F_Alpha (F_Alpha only without --mask_dir)')
    p.add_argument('--save_path', required=True, help='the checkpoint to write')
    p.add_argument('--mask_dir', default=None, help='foreground masks, one file per frame (default: F_Alpha decides)')
    p.add_argument('--iters', type=int, default=10000)
    p.add_argument('--batch', type=int, default=10000)
    p.add_argument('--seed', type=int, default=0)
    add_frame_arguments(p, frames=False)
    return p


def run(args, device=None):
    from . import atlas, formats
    device = torch.device('cuda') if device is None else device
    config = atlas.load_atlas_config(args.atlas_config_path)
    models_cfg = config.get('models', {})
    if 'FG_UV_Mapping' not in models_cfg:
        raise formats.FormatError('atlas config: models.FG_UV_Mapping is missing')
    spec = models_cfg.get('FG_UV_Mapping_Inverse')
    if spec is None:
        spec = dict(copy.deepcopy(dict(models_cfg['FG_UV_Mapping'])), output_dim=3)
    names = ('FG_UV_Mapping',) if args.mask_dir else ('FG_UV_Mapping', 'F_Alpha')
    models = atlas.load_atlas_models(config, args.atlas_model_path, device=device, names=names)
    T = atlas.number_of_frames(config, args.num_frames)
    W, H = int(config['datasets']['res_x']), int(config['datasets']['res_y'])
    ckpt = formats._load(args.atlas_model_path)

    torch.manual_seed(args.seed)                                   # the initialisation and the samples
    inverse = atlas.build_network(spec)
    if not isinstance(inverse, atlas.CoordMLP):
        raise NotImplementedError('models.FG_UV_Mapping_Inverse: pe_type hash_encoding has no gradient path')
    started_from = 'a fresh initialisation'
    if 'FG_UV_Mapping_Inverse' in ckpt:
        try:
            inverse.load_state_dict(ckpt['FG_UV_Mapping_Inverse'])
            started_from = "the checkpoint's FG_UV_Mapping_Inverse"
        except RuntimeError:
            pass                                                   # another architecture: it is replaced
    inverse = inverse.to(device)
    select = atlas.load_mask_frames(args.mask_dir, W, H, T) if args.mask_dir else models['F_Alpha']
    result = atlas.fit_inverse_mapping(models['FG_UV_Mapping'], inverse, select, W, H, T, iters=args.iters, batch=args.batch)

    out = dict(ckpt)
    out['FG_UV_Mapping_Inverse'] = {k: v.detach().cpu() for k, v in inverse.state_dict().items()}
    os.makedirs(os.path.dirname(os.path.abspath(args.save_path)), exist_ok=True)
    torch.save(out, args.save_path)
    used = copy.deepcopy(_plain(config))
    used.setdefault('models', {})['FG_UV_Mapping_Inverse'] = _plain(spec)
    config_path = os.path.splitext(args.save_path)[0] + '.yml'
    import yaml
    with open(config_path, 'w') as f:
        yaml.safe_dump(used, f, sort_keys=False)
    hist = result['loss_history']
    print(f'{len(hist)} steps from {started_from} ({result["steps_skipped"]} without a foreground row skipped): loss '
          f'{hist[0] if hist else float("nan"):.6f} -> {hist[-1] if hist else float("nan"):.6f}; round trip on '
          f'{result["holdout_rows"]} held-out foreground samples: mean {result["roundtrip_mean_px"]:.3f} px, max '
          f'{result["roundtrip_max_px"]:.3f} px')
    print(f'save to {args.save_path} and {config_path}')
    result.update(save_path=args.save_path, config_path=config_path)
    return result


def _plain(obj):
    """dict subclasses and tuples of a loaded config -> what yaml.safe_dump writes"""
    if isinstance(obj, dict):
        return {k: _plain(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return [_plain(v) for v in obj]
    return obj


def main(argv=None):
    run(build_parser().parse_args(argv))


if __name__ == '__main__':
    main()
