#!/usr/bin/env python
"""Edge adherence of a folder of images to a folder of control images, after the fact.
    python tools/edge_adherence.py --control DIR --images DIR [--edge_tolerance 1] [--canny_low 100] [--canny_high 200] [--batch 16]
Image i (PNG / JPEG, sorted by name) is scored against control file i mod len(control): the rule generate_onestep.py --control_images
uses.  The control's edge set is its pixels with any channel >= 128; the image's edge set is its Canny map (sid_lsg_amd.edges.canny).
An image and its control must have equal sizes (a pair that differs is refused by name; nothing is resampled here).  The result is the
JSON of generate_onestep.py --control_adherence 1 (`options`, `per_image` keyed by image file name, `mean`) on stdout."""
import contextlib
import json
import os
import sys

import click
import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sid_lsg_amd import edges  # noqa: E402

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


def pairs(control, images):
    """-> [(image path, image [H, W, 3], control [H, W, 3])], sizes checked by name."""
    for i, t in enumerate(images):
        c = control[i % len(control)]
        a, b = load(t), load(c)
        if a.shape != b.shape:
            raise click.UsageError(f'{t} is {a.shape[1]} x {a.shape[0]} but its control image {c} is {b.shape[1]} x {b.shape[0]}: equal sizes are required')
        if edges.hysteresis_lds_bytes(a.shape[0], a.shape[1]) > edges.HYST_LDS_MAX:
            raise click.UsageError(f'{t} is {a.shape[1]} x {a.shape[0]}: the Canny hysteresis keeps both bit planes of an image on chip, '
                                   f'{edges.hysteresis_lds_bytes(a.shape[0], a.shape[1])} bytes here against a limit of {edges.HYST_LDS_MAX} (768 x 768)')
        yield t, a, b


@click.command(help=__doc__)
@click.option('--control', type=str, required=True, metavar='DIR', help='Control images (edge maps)')
@click.option('--images', type=str, required=True, metavar='DIR', help='Images to score')
@click.option('--edge_tolerance', type=int, default=1, show_default=True, help='A hit lies within this many pixels (Chebyshev) of an edge of the other set')
@click.option('--canny_low', type=int, default=100, show_default=True, help='Lower Canny threshold for the images')
@click.option('--canny_high', type=int, default=200, show_default=True, help='Upper Canny threshold for the images')
@click.option('--batch', type=click.IntRange(min=1), default=16, show_default=True, help='Images per pass')
def main(control, images, edge_tolerance, canny_low, canny_high, batch):
    control_files, image_files_ = image_files('--control', control), image_files('--images', images)
    for flag, v in (('--canny_low', canny_low), ('--canny_high', canny_high), ('--edge_tolerance', edge_tolerance)):
        if v < 0:
            raise click.UsageError(f'{flag} {v}: cannot be negative')
    if canny_low > canny_high:
        raise click.UsageError(f'--canny_low {canny_low} is above --canny_high {canny_high}')
    if edge_tolerance > edges.MAX_TOLERANCE:
        raise click.UsageError(f'--edge_tolerance {edge_tolerance}: at most {edges.MAX_TOLERANCE} pixels')
    todo = list(pairs(control_files, image_files_))                 # every size is checked before the GPU is touched
    dev = torch.device('cuda:0')
    per_image, run = {}, []

    def flush():
        if run:
            out = torch.from_numpy(np.stack([r[1] for r in run])).to(dev)
            ctl = edges.pack(torch.from_numpy(np.stack([r[2] for r in run])).to(dev))
            for r, row in zip(run, edges.score_batch(ctl, out, canny_low, canny_high, edge_tolerance)):
                per_image[os.path.basename(r[0])] = row
            run.clear()
    with contextlib.redirect_stdout(sys.stderr):                    # notices go to stderr: stdout carries the JSON alone
        for item in todo:
            if run and (len(run) == batch or item[1].shape != run[0][1].shape):
                flush()
            run.append(item)
        flush()
    report = dict(options=dict(control=control, images=images, edge_tolerance=edge_tolerance, canny_low=canny_low, canny_high=canny_high),
                  per_image=per_image, mean=edges.aggregate(per_image))
    print(json.dumps(report, indent=1))
    return report


if __name__ == '__main__':
    main()
