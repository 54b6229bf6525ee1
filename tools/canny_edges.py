#!/usr/bin/env python
"""Canny control images for a folder of photographs: what ControlNet's Canny annotator writes, made on the device.
    python tools/canny_edges.py --images DIR --out DIR --resolution N [--canny_low 100] [--canny_high 200] [--batch 16]
Every PNG / JPEG file of --images (sorted by name) is loaded by the rule of generate_onestep.py's load_init_image (RGB, centre crop to a
square, LANCZOS resize to N x N); its edge map (sid_lsg_amd.edges.canny: OpenCV's Canny(img, low, high) restated, aperture 3, L1
gradient) is written to --out as <name>.png, 255 in all three channels on an edge: a folder `--control_images` takes as it is."""
import os
import sys

import click
import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from generate_onestep import load_init_image  # noqa: E402
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


def check_canny(low, high):
    """The usage errors of --canny_low / --canny_high, by name."""
    for flag, v in (('--canny_low', low), ('--canny_high', high)):
        if v < 0:
            raise click.UsageError(f'{flag} {v}: cannot be negative')
    if low > high:
        raise click.UsageError(f'--canny_low {low} is above --canny_high {high}')


def check_resolution(resolution):
    if edges.hysteresis_lds_bytes(resolution, resolution) > edges.HYST_LDS_MAX:
        raise click.UsageError(f'--resolution {resolution}: the Canny hysteresis keeps both bit planes of an image on chip, '
                               f'{edges.hysteresis_lds_bytes(resolution, resolution)} bytes here against a limit of {edges.HYST_LDS_MAX} (768 x 768)')


@click.command(help=__doc__)
@click.option('--images', type=str, required=True, metavar='DIR', help='Photographs of any size')
@click.option('--out', type=str, required=True, metavar='DIR', help='Where the control PNGs go')
@click.option('--resolution', type=click.IntRange(min=1), required=True, help='Side of the control images')
@click.option('--canny_low', type=int, default=100, show_default=True, help='Lower threshold')
@click.option('--canny_high', type=int, default=200, show_default=True, help='Upper threshold')
@click.option('--batch', type=click.IntRange(min=1), default=16, show_default=True, help='Images per launch')
def main(images, out, resolution, canny_low, canny_high, batch):
    import PIL.Image
    files = image_files('--images', images)
    check_canny(canny_low, canny_high)
    check_resolution(resolution)
    stems = [os.path.splitext(os.path.basename(f))[0] for f in files]
    twice = sorted({s for s in stems if stems.count(s) > 1})
    if twice:
        raise click.UsageError(f'--images {images}: {twice[0]!r} names more than one file; the control images are written as <name>.png')
    dev = torch.device('cuda:0')
    os.makedirs(out, exist_ok=True)
    total = 0
    for i in range(0, len(files), batch):
        pix = np.stack([load_init_image(f, resolution) for f in files[i:i + batch]])
        maps = edges.canny(torch.from_numpy(pix).to(dev), canny_low, canny_high, rgb=True)
        rgb = maps.rgb_u8().cpu().numpy()
        for stem, img in zip(stems[i:i + batch], rgb):
            PIL.Image.fromarray(img).save(os.path.join(out, stem + '.png'))
            total += int(img[..., 0].astype(bool).sum())
    print(f'{len(files)} control image(s) of {resolution} x {resolution} written to "{out}": Canny {canny_low} / {canny_high}, {total} edge pixels')


if __name__ == '__main__':
    main()
