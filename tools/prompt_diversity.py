#!/usr/bin/env python
"""Per-prompt diversity of a folder of images, after the fact: the all-pairs LPIPS among the K samples of every prompt.
    python tools/prompt_diversity.py --images DIR --group K --lpips_vgg SPEC --lpips_lin SPEC [--prompts FILE] [--batch N]
The files of DIR (PNG / JPEG, sorted by name) are read in consecutive runs of K: one run is one group, the K samples one prompt gave
under K seeds -- the layout generate_onestep.py --seeds_per_prompt K writes.  All files must have one size, and their count must be a
multiple of K; both are refused by name otherwise, before the GPU is touched.  --prompts: the prompt file of the run (group g is
labelled with line g mod len).  --batch: images per scoring call, rounded down to whole groups (at least one).  Everything runs on
sid_lsg_amd.fidelity's HIP kernels: VGG16 once per image, all pairs of a group in one launch per tap.  The result is the JSON of
generate_onestep.py --diversity 1 (`options`, `per_prompt` keyed by group index, `mean`) on stdout; notices go to stderr."""
import contextlib
import json
import os
import sys

import click
import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sid_lsg_amd import diversity, fidelity  # noqa: E402

EXTENSIONS = ('.png', '.jpg', '.jpeg')


def image_files(option, path):
    """The PNG / JPEG files of a directory, sorted by name."""
    if not os.path.isdir(path):
        raise click.UsageError(f'{option} {path}: not a directory')
    files = sorted(f for f in os.listdir(path) if f.lower().endswith(EXTENSIONS) and os.path.isfile(os.path.join(path, f)))
    if not files:
        raise click.UsageError(f'{option} {path}: no PNG or JPEG files')
    return [os.path.join(path, f) for f in files]


def load(path):
    import PIL.Image
    with PIL.Image.open(path) as im:
        return np.ascontiguousarray(np.asarray(im.convert('RGB'), dtype=np.uint8))


def group_files(files, K):
    """Consecutive runs of K files -> [[paths of group 0], ..]; a count that is no multiple of K is refused."""
    if len(files) % K:
        raise click.UsageError(f'--images: {len(files)} PNG or JPEG files are not a multiple of --group {K}')
    return [files[i:i + K] for i in range(0, len(files), K)]


def check_sizes(files):
    """(width, height) shared by every file; refused by name otherwise.  Only the headers are read."""
    import PIL.Image
    size = None
    for path in files:
        with PIL.Image.open(path) as im:
            if size is None:
                size, first = im.size, path
            elif im.size != size:
                raise click.UsageError(f'{path} is {im.size[0]} x {im.size[1]} but {first} is {size[0]} x {size[1]}: equal sizes are required')
    if size[0] < 16 or size[1] < 16:
        raise click.UsageError(f'{first} is {size[0]} x {size[1]}: LPIPS-VGG needs at least 16 x 16 pixels')
    return size


@click.command(help=__doc__)
@click.option('--images', type=str, required=True, metavar='DIR', help='Images to score: consecutive runs of --group files (sorted by name) are the samples of one prompt')
@click.option('--group', type=click.IntRange(min=2, max=fidelity.GROUP_MAX), required=True, metavar='K', help='Samples per prompt')
@click.option('--lpips_vgg', type=str, default=None, metavar='SPEC', help="A torch.save'd torchvision VGG16 state dict, or random:lpips-vgg[:seed]")
@click.option('--lpips_lin', type=str, default=None, metavar='SPEC', help="The lpips package's lin weights (vgg.pth), or random:lpips-vgg[:seed]")
@click.option('--prompts', type=str, default=None, metavar='FILE', help='Prompt file of the run, one per line: group g is labelled with line g mod len')
@click.option('--batch', type=click.IntRange(min=1), default=16, show_default=True, help='Images per scoring call (whole groups; at least one group)')
def main(images, group, lpips_vgg, lpips_lin, prompts, batch):
    try:
        fidelity.check_specs(lpips_vgg, lpips_lin)
    except ValueError as e:
        raise click.UsageError(str(e))
    files = image_files('--images', images)
    groups = group_files(files, group)
    check_sizes(files)                                              # every refusal comes before the GPU is touched
    captions = None
    if prompts is not None:
        if not os.path.isfile(prompts):
            raise click.UsageError(f'--prompts {prompts}: not a file')
        with open(prompts, 'rt') as f:
            captions = [line.strip() for line in f if line.strip()]
        if not captions:
            raise click.UsageError(f'--prompts {prompts}: no prompts')
    dev = torch.device('cuda:0')
    per_prompt = {}
    step = max(1, batch // group)
    with contextlib.redirect_stdout(sys.stderr):                    # notices go to stderr: stdout carries the JSON alone
        net = fidelity.load_lpips(lpips_vgg, lpips_lin, dev)
        for g0 in range(0, len(groups), step):
            run = groups[g0:g0 + step]
            x = torch.from_numpy(np.stack([load(p) for grp in run for p in grp])).to(dev).permute(0, 3, 1, 2).contiguous()
            for g, (grp, row) in enumerate(zip(run, diversity.score_groups(x, group, net)), start=g0):
                label = {} if captions is None else {'prompt': captions[g % len(captions)]}
                per_prompt[str(g)] = dict(**label, files=[os.path.basename(p) for p in grp], **row)
    report = dict(options=dict(images=images, group=group, prompts=prompts, lpips_vgg=lpips_vgg, lpips_lin=lpips_lin), per_prompt=per_prompt,
                  mean=diversity.aggregate(per_prompt))
    print(json.dumps(report, indent=1))
    return report


if __name__ == '__main__':
    main()
