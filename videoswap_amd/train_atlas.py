"""python -m videoswap_amd.train_atlas -opt <atlas yml> — train a layered neural atlas on the GPU.

What train_atlas.py does with the reference's YAML (e.g. 4022_4_atlas_rabbit_inv_fp32.yml): build the five networks, read
the frames, masks and flows (atlas_fit.load_training_data), pre-train both mapping networks when
train.pretrain_UV_mapping_iter > 0, run atlas_fit.fit_atlas for train.total_iter steps, log every logger.print_freq steps,
report the reconstruction PSNR of render_atlas every val.val_freq steps, and write models_<iter>.pth with the reference's
five keys every logger.save_checkpoint_freq steps (and after the last step) under <root>/<name>/models, which
atlas.load_atlas_models and every atlas tool read.  Not done here: save_mask_flow's videos, annotate_validation,
accelerate (one GPU, fp32), the atlas and edit images of evaluate_model (render_atlas / edit_atlas write them on demand).
"""
import argparse
import os
import random

import torch


def build_parser():
    p = argparse.ArgumentParser(prog='python -m videoswap_amd.train_atlas', description=__doc__.split('\n')[0])
    p.add_argument('-opt', required=True, help='the atlas YAML')
    p.add_argument('--root', default='experiments', help='experiments directory (default: experiments)')
    p.add_argument('--total_iter', type=int, default=None, help='overrides train.total_iter')
    p.add_argument('--device', default=None)
    return p


def save_checkpoint(path, models, inverse):
    state = {k: {n: v.detach().cpu() for n, v in models[k].state_dict().items()} for k in ('F_Atlas', 'FG_UV_Mapping', 'BG_UV_Mapping', 'F_Alpha')}
    if inverse is not None:
        state['FG_UV_Mapping_Inverse'] = {n: v.detach().cpu() for n, v in inverse.state_dict().items()}
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    torch.save(state, path)


def run(args, device=None, log=print):
    from . import atlas, atlas_fit
    opt = atlas.load_atlas_config(args.opt)
    device = torch.device(device or args.device or ('cuda' if torch.cuda.is_available() else 'cpu'))
    seed = opt.get('manual_seed')
    seed = random.randint(1, 10000) if seed is None else seed
    random.seed(seed)
    torch.manual_seed(seed)
    # in the reference's order of construction, so that one seed gives the coordinate networks its initial weights
    models = {k: atlas.build_network(opt['models'][k]).to(device) for k in ('FG_UV_Mapping', 'BG_UV_Mapping', 'F_Alpha', 'F_Atlas')}
    inverse = atlas.build_network(opt['models']['FG_UV_Mapping_Inverse']).to(device) if 'FG_UV_Mapping_Inverse' in opt['models'] else None
    data = atlas_fit.load_training_data(opt['datasets'])
    H, W, _, T = data['video_frames'].shape
    train_opt = opt['train']
    if train_opt.get('pretrain_UV_mapping_iter', 0) > 0:
        for k in ('FG_UV_Mapping', 'BG_UV_Mapping'):
            _, loss = atlas_fit.pretrain_mapping(models[k], train_opt['uv_mapping_scale'], W, H, T,
                                                 pretrain_iters=train_opt['pretrain_UV_mapping_iter'])
            log(f'Finish pretrain {k} with final loss: {loss:.4f}')
    total = int(train_opt['total_iter'] if args.total_iter is None else args.total_iter)
    model_dir = os.path.join(args.root, opt['name'], 'models')
    print_freq, val_freq = int(opt['logger']['print_freq']), int(opt['val']['val_freq'])
    save_freq = int(opt['logger']['save_checkpoint_freq'])
    frames = data['video_frames'].permute(3, 0, 1, 2)
    saved = []

    def on_step(step, loss_dict):
        it = step + 1
        if it % print_freq == 0:
            log(f'[iter {it}] ' + ' '.join(f'{k}: {float(v.detach()):.4e}' for k, v in loss_dict.items()))
        if it % val_freq == 0:
            psnr = atlas.atlas_psnr(atlas.render_atlas(models, W, H, T)['reconstruction'], frames)[1]
            log(f'Validation Reconstruction PSNR: {psnr:.4f}')
        if it % save_freq == 0 or it == total:
            saved.append(os.path.join(model_dir, f'models_{it}.pth'))
            save_checkpoint(saved[-1], models, inverse)
            log(f'Save models to {saved[-1]}')

    history, last = atlas_fit.fit_atlas(models, data, train_opt, total, batch=int(opt['datasets']['sample_batch_size']), inverse=inverse,
                                        on_step=on_step)
    return dict(history=history, loss_dict=last, checkpoints=saved)


def main(argv=None):
    run(build_parser().parse_args(argv))


if __name__ == '__main__':
    main()
