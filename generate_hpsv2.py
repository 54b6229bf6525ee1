#!/usr/bin/env python
"""HPSv2 benchmark of a distilled generator (counterpart of the reference's `generate_hpsv2.py`).

    torchrun --standalone --nproc_per_node=8 generate_hpsv2.py --network runs/00000-.../network-snapshot-1.000000-000500.pkl \\
        --outdir out_hps --batch 16 --repo_id /models/stable-diffusion-v1-5 --hps_prompts /data/hpsv2/benchmark \\
        --hps_checkpoint /models/HPS_v2_compressed.pt

The reference's loop (`generate_hpsv2.py:157-191`): for each of the four styles of the HPSv2 benchmark (anime, concept-art, paintings,
photo), image `seed` is generated from prompt `seed` of that style and the latent of torch.Generator(seed) -- the same latent for
every style -- in rank-strided batches, and written by PIL with its default quality as `<outdir>/<style>/<seed:05d>.jpg`; then the
directory is scored.  Here the prompts come from `--hps_prompts DIR` (anime.json, concept-art.json, paintings.json, photo.json: the
package's benchmark layout) and the scorer is `--hps_checkpoint` (HPS_v2_compressed.pt, or any checkpoint in open_clip's layout) on
the HIP CLIP towers (sid_lsg_amd.clip.load_open_clip, sid_lsg_amd.hps); neither the hpsv2 package nor open_clip is needed.  The
score is computed from the JPEG files read back, as `hpsv2.evaluate` does; rank 0 prints the table and writes `<outdir>/hpsv2.json`.
`--score_only` scores an existing `--outdir` without generating.  `--network teacher` samples the teacher of `--repo_id` as
generate_onestep.py does.
"""
import json
import os

import click
import numpy as np
import torch

from generate_onestep import StackedRandomGenerator, load_generator, parse_int_list, sample_images, teacher_options, to_uint8_nhwc
from sid_lsg_amd import distributed as dist
from sid_lsg_amd import hps
from sid_lsg_amd.sd_util import TEACHER, TEACHER_CFG, TEACHER_STEPS


def resolve_scorer_options(repo_id, hps_prompts, hps_checkpoint, hps_tokenizer, hps_arch):
    """-> (prompts by style, checkpoint, tokenizer directory, arch); refuses what is missing before any network is loaded."""
    if not hps_prompts:
        raise click.UsageError('--hps_prompts DIR is required: the HPSv2 benchmark prompts (anime.json, concept-art.json, paintings.json, photo.json)')
    try:
        prompts = hps.benchmark_prompts(hps_prompts)
    except (OSError, ValueError) as e:
        raise click.UsageError(f'--hps_prompts: {e}')
    if not hps_checkpoint or not os.path.isfile(hps_checkpoint):
        raise click.UsageError(f'--hps_checkpoint {hps_checkpoint!r}: a local checkpoint in open_clip\'s layout is needed (HPS_v2_compressed.pt)')
    tokenizer = hps_tokenizer if hps_tokenizer is not None else os.path.join(repo_id, 'tokenizer')
    for f in ('vocab.json', 'merges.txt'):
        if not os.path.isfile(os.path.join(tokenizer, f)):
            raise click.UsageError(f'--hps_tokenizer {tokenizer}: {f} is missing (the tokenizer/ directory of a Stable Diffusion model has it)')
    return prompts, hps_checkpoint, tokenizer, hps_arch


def check_seeds(seeds, prompts):
    """The prompt of seed i is prompts[style][i]: every seed must index every style's list."""
    for style, p in prompts.items():
        bad = [s for s in seeds if not 0 <= s < len(p)]
        if bad:
            raise click.UsageError(f'--seeds: seed {bad[0]} has no prompt in {style}.json ({len(p)} prompts)')


@click.command()
@click.option('--network', 'network_pkl', type=str, default=None, metavar='PATH', help=f'Network snapshot pickle, or "{TEACHER}": sample the UNet of --repo_id itself')
@click.option('--outdir', type=str, required=True, metavar='DIR', help='Where to save the output images')
@click.option('--seeds', type=parse_int_list, default='0-799', show_default=True, metavar='LIST', help='Random seeds = prompt indices (e.g. 1,2,5-10)')
@click.option('--subdirs', is_flag=True, help='Create subdirectory for every 1000 seeds')
@click.option('--batch', 'max_batch_size', type=click.IntRange(min=1), default=16, show_default=True, help='Maximum batch size')
@click.option('--num', 'num_fid_samples', type=click.IntRange(min=1), default=800, show_default=True, help='Maximum number of images per style')
@click.option('--init_timestep', type=click.IntRange(min=0), default=625, show_default=True, help='t_init, in [0,999]')
@click.option('--repo_id', type=str, default='runwayml/stable-diffusion-v1-5', show_default=True, help='Local diffusers directory, random:<arch> or random:<arch>:v')
@click.option('--resolution', type=click.IntRange(min=8), default=512, show_default=True, help='Image resolution (latent = resolution / 8) (not a reference option)')
@click.option('--num_steps_eval', type=click.IntRange(min=0), default=1, show_default=True, help='Generation steps (1 = one-step) (not a reference option)')
@click.option('--text_encoder', type=click.Choice(['torch', 'hip']), default=None, help='CLIP text encoder of the generator  [default: $SIDLSG_TEXT_ENCODER, else torch] (not a reference option)')
@click.option('--teacher_steps', type=click.IntRange(min=1), default=None, help=f'DDIM steps of --network {TEACHER}  [default: {TEACHER_STEPS}]')
@click.option('--guidance_scale', type=float, default=None, help=f'Classifier-free guidance scale of --network {TEACHER}  [default: {TEACHER_CFG}]')
@click.option('--hps_prompts', type=str, default=None, metavar='DIR', help='HPSv2 benchmark prompts: anime.json, concept-art.json, paintings.json, photo.json')
@click.option('--hps_checkpoint', type=str, default=None, metavar='FILE', help='HPS_v2_compressed.pt, or any checkpoint in open_clip\'s layout (.pt / .bin / .safetensors)')
@click.option('--hps_tokenizer', type=str, default=None, metavar='DIR', help='vocab.json / merges.txt of the scorer  [default: <repo_id>/tokenizer]')
@click.option('--hps_arch', type=str, default='ViT-H-14', show_default=True, help='open_clip architecture of --hps_checkpoint')
@click.option('--score_only', is_flag=True, help='Score the JPEG files already in --outdir; generate nothing')
def main(network_pkl, outdir, seeds, subdirs, max_batch_size, num_fid_samples, init_timestep, repo_id, resolution, num_steps_eval, text_encoder,
         teacher_steps, guidance_scale, hps_prompts, hps_checkpoint, hps_tokenizer, hps_arch, score_only):
    if resolution % 8:
        raise click.BadParameter(f'{resolution}: must be a multiple of 8', param_hint='--resolution')
    if not score_only and not network_pkl:
        raise click.UsageError('--network is required unless --score_only is given')
    teacher = None if score_only else teacher_options(network_pkl, teacher_steps, guidance_scale)
    all_prompts, checkpoint, tokenizer_dir, arch = resolve_scorer_options(repo_id, hps_prompts, hps_checkpoint, hps_tokenizer, hps_arch)
    seeds = seeds[:num_fid_samples]
    check_seeds(seeds, all_prompts)
    dist.init()
    device = torch.device('cuda')
    rank, world = dist.get_rank(), dist.get_world_size()

    if not score_only:
        num_batches = ((len(seeds) - 1) // (max_batch_size * world) + 1) * world
        rank_batches = torch.as_tensor(seeds).tensor_split(num_batches)[rank::world]
        if world > 1 and rank != 0:
            torch.distributed.barrier()                    # rank 0 touches the files first
        net = load_generator(network_pkl, repo_id, device, text_encoder, teacher)
        if world > 1 and rank == 0:
            torch.distributed.barrier()
        lat = resolution // 8
        for style in hps.STYLES:
            dist.print0(f'Generating {len(seeds)} images to "{outdir}/{style}"...')
            for batch_seeds in rank_batches:
                if world > 1:
                    torch.distributed.barrier()
                if len(batch_seeds) == 0:
                    continue
                batch_seeds = [int(s) for s in batch_seeds]
                z = StackedRandomGenerator(device, batch_seeds).randn([len(batch_seeds), 4, lat, lat], device=device)
                images = sample_images(net, z, [all_prompts[style][s] for s in batch_seeds], resolution, teacher, None, init_timestep, num_steps_eval)
                for seed, img in zip(batch_seeds, to_uint8_nhwc(images)):
                    path = hps.image_path(outdir, style, seed, subdirs)
                    os.makedirs(os.path.dirname(path), exist_ok=True)
                    with open(path, 'wb') as f:
                        f.write(hps.jpeg_bytes(np.ascontiguousarray(img)))
        del net
        if world > 1:
            torch.distributed.barrier()

    from sid_lsg_amd.clip import load_open_clip
    dist.print0(f'Scoring "{outdir}" with "{checkpoint}" ({arch})...')
    det = load_open_clip(checkpoint, tokenizer_dir, device, arch=arch)
    mine = hps.score_directory(det, outdir, all_prompts, seeds, subdirs=subdirs, batch=max_batch_size, rank=rank, world=world)
    scores = hps.gather_scores(mine, seeds, rank, world, device)
    result = hps.aggregate(scores)
    if rank == 0:
        print(hps.format_table(result))
        with open(os.path.join(outdir, hps.RESULT_FILE), 'w') as f:
            json.dump(dict(result, num_images={s: len(v) for s, v in scores.items()}, checkpoint=os.path.basename(checkpoint), arch=arch), f, indent=2)
    if world > 1:
        torch.distributed.barrier()
    dist.print0('Done.')


if __name__ == '__main__':
    main()
