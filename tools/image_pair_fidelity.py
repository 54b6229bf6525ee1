#!/usr/bin/env python
"""PSNR, SSIM and LPIPS of a folder of images against the folder they started from, after the fact.
    python tools/image_pair_fidelity.py --ref DIR --test DIR [--masks DIR] [--lpips_vgg SPEC --lpips_lin SPEC] [--batch 16]
Test file i (PNG / JPEG, sorted by name) pairs with ref file i mod len(ref): the rule generate_onestep.py --init_images uses, so
--ref is that run's init images (already cropped to the output size: a pair of different sizes is refused by name, nothing is
resampled here) and --test its output folder.  --masks: one mask file or one per ref file, kept = < 128, the same sizes; the `_keep`
figures are those of the kept region.  LPIPS-VGG runs when both --lpips_* are given (a torchvision VGG16 state dict and the lpips
package's lin weights, or random:lpips-vgg[:seed] for both).  Everything runs on sid_lsg_amd.fidelity's HIP kernels.  The result is
the JSON of generate_onestep.py --fidelity 1 (`options`, `per_image` keyed by test file name, `mean`) on stdout."""
import contextlib
import json
import os
import sys

import click
import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sid_lsg_amd import fidelity  # noqa: E402

EXTENSIONS = ('.png', '.jpg', '.jpeg')


def image_files(option, path):
    """The PNG / JPEG files of a directory, sorted by name."""
    if not os.path.isdir(path):
        raise click.UsageError(f'{option} {path}: not a directory')
    files = sorted(f for f in os.listdir(path) if f.lower().endswith(EXTENSIONS) and os.path.isfile(os.path.join(path, f)))
    if not files:
        raise click.UsageError(f'{option} {path}: no PNG or JPEG files')
    return [os.path.join(path, f) for f in files]


def load(path, mode):
    import PIL.Image
    with PIL.Image.open(path) as im:
        return np.ascontiguousarray(np.asarray(im.convert(mode), dtype=np.uint8))


def pairs(ref, test, masks):
    """-> [(test path, test [H, W, 3], ref [H, W, 3], mask [H, W] or None)], sizes checked by name."""
    for i, t in enumerate(test):
        r = ref[i % len(ref)]
        a, b = load(t, 'RGB'), load(r, 'RGB')
        if a.shape != b.shape:
            raise click.UsageError(f'{t} is {a.shape[1]} x {a.shape[0]} but its reference {r} is {b.shape[1]} x {b.shape[0]}: equal sizes are required')
        m = None
        if masks is not None:
            mp = masks[i % len(masks)]
            m = load(mp, 'L')
            if m.shape != a.shape[:2]:
                raise click.UsageError(f'{mp} is {m.shape[1]} x {m.shape[0]} but {t} is {a.shape[1]} x {a.shape[0]}: equal sizes are required')
        if a.shape[0] < 11 or a.shape[1] < 11:
            raise click.UsageError(f'{t} is {a.shape[1]} x {a.shape[0]}: SSIM needs at least 11 x 11 pixels')
        yield t, a, b, m


@click.command(help=__doc__)
@click.option('--ref', type=str, required=True, metavar='DIR', help='Reference (init) images')
@click.option('--test', type=str, required=True, metavar='DIR', help='Images to score')
@click.option('--masks', type=str, default=None, metavar='DIR', help='Mask files: one for all, or one per reference image; kept = < 128')
@click.option('--lpips_vgg', type=str, default=None, metavar='SPEC', help="A torch.save'd torchvision VGG16 state dict, or random:lpips-vgg[:seed]")
@click.option('--lpips_lin', type=str, default=None, metavar='SPEC', help="The lpips package's lin weights (vgg.pth), or random:lpips-vgg[:seed]")
@click.option('--batch', type=click.IntRange(min=1), default=16, show_default=True, help='Pairs per pass')
def main(ref, test, masks, lpips_vgg, lpips_lin, batch):
    ref_files, test_files = image_files('--ref', ref), image_files('--test', test)
    mask_files = None
    if masks is not None:
        mask_files = image_files('--masks', masks)
        if len(mask_files) not in (1, len(ref_files)):
            raise click.UsageError(f'--masks {masks}: {len(mask_files)} PNG or JPEG files, expected 1 or one per reference image ({len(ref_files)})')
    if lpips_vgg is not None or lpips_lin is not None:
        try:
            fidelity.check_specs(lpips_vgg, lpips_lin)
        except ValueError as e:
            raise click.UsageError(str(e))
    todo = list(pairs(ref_files, test_files, mask_files))          # every size is checked before the GPU is touched
    dev = torch.device('cuda:0')
    net = fidelity.load_lpips(lpips_vgg, lpips_lin, dev) if lpips_vgg is not None else None
    per_image, run = {}, []

    def flush():
        if run:
            a = torch.from_numpy(np.stack([r[1] for r in run])).to(dev).permute(0, 3, 1, 2).contiguous()
            b = torch.from_numpy(np.stack([r[2] for r in run])).to(dev).permute(0, 3, 1, 2).contiguous()
            m = None if mask_files is None else torch.from_numpy(np.stack([r[3] for r in run])).to(dev)
            for r, row in zip(run, fidelity.score_batch(b, a, m, net)):
                per_image[os.path.basename(r[0])] = row
            run.clear()
    with contextlib.redirect_stdout(sys.stderr):                    # notices go to stderr: stdout carries the JSON alone
        for item in todo:
            if run and (len(run) == batch or item[1].shape != run[0][1].shape):
                flush()
            run.append(item)
        flush()
    report = dict(options=dict(ref=ref, test=test, masks=masks, lpips_vgg=lpips_vgg, lpips_lin=lpips_lin), per_image=per_image,
                  mean=fidelity.aggregate(per_image))
    print(json.dumps(report, indent=1))
    return report


if __name__ == '__main__':
    main()
