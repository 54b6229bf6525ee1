#!/usr/bin/env python
"""KID and / or CMMD between two folders of PNG / JPEG images, e.g. a real set and a generate_onestep.py run scored after the fact.
    python tools/image_set_distance.py --real DIR --fake DIR [--kid --detector FILE] [--cmmd --clip DIR] [--batch 64]
--kid: the Inception detector of FID (a TorchScript file, a state-dict .pth or random:inception-v3; metrics.load_detector); the real images as stored, the generated ones resized
to 256 x 256 with Pillow's LANCZOS arithmetic, as the metrics treat them; 100 subsets of at most 1000 -- what `kid30k_full` reports.  --cmmd: the image tower of a local CLIP directory in
the Hugging Face layout (ViT-L/14-336 in the published CMMD; or 'random:clip-<arch>'), images straight from their own sizes --
what `cmmd30k_full` reports.  Both sums run on sidlsg_pair_kernel_sums (fp32 MFMA, fp64 accumulation)."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sid_lsg_amd import metrics  # noqa: E402

EXTENSIONS = ('.png', '.jpg', '.jpeg')


def image_files(root):
    """Every PNG / JPEG file below `root`, sorted by path."""
    out = [os.path.join(d, f) for d, _, files in os.walk(root) for f in files if f.lower().endswith(EXTENSIONS)]
    if not out:
        raise SystemExit(f'{root}: no {" / ".join(EXTENSIONS)} files')
    return sorted(out)


def features(files, detector, dev, batch, size=None):
    """[len(files), F] fp32 on the device: the files through PIL as RGB uint8, in runs of equally sized images of at most `batch`,
    resized to size x size first when `size` is given, through `detector`."""
    import PIL.Image
    out, run = [], []

    def flush():
        if run:
            imgs = torch.stack(run).to(dev)
            if size is not None:
                imgs = metrics.resize_for_detector(imgs, size)
            with torch.no_grad():
                out.append(detector(imgs, return_features=True).float())
            run.clear()
    for p in files:
        img = torch.from_numpy(np.array(PIL.Image.open(p).convert('RGB'))).permute(2, 0, 1).contiguous()
        if run and (len(run) == batch or img.shape != run[0].shape):
            flush()
        run.append(img)
    flush()
    return torch.cat(out).contiguous()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--real', required=True)
    ap.add_argument('--fake', required=True)
    ap.add_argument('--kid', action='store_true')
    ap.add_argument('--detector', help='--kid: the Inception detector of FID: a TorchScript file, a state-dict .pth, or random:inception-v3')
    ap.add_argument('--cmmd', action='store_true')
    ap.add_argument('--clip', help="--cmmd: a CLIP directory in the Hugging Face layout, or 'random:clip-<arch>'")
    ap.add_argument('--batch', type=int, default=64)
    a = ap.parse_args(argv)
    if not (a.kid or a.cmmd):
        ap.error('nothing to compute: pass --kid and / or --cmmd')
    if a.kid and not a.detector:
        ap.error('--kid needs --detector')
    if a.cmmd and not (a.clip and metrics.is_clip_spec(a.clip)):
        ap.error(f'--cmmd needs --clip to be a local CLIP directory or random:clip-<arch> (got {a.clip!r})')
    real, fake = image_files(a.real), image_files(a.fake)
    dev = torch.device('cuda:0')
    results = {}
    if a.kid:
        det = metrics.load_detector(a.detector, dev)
        results['kid'] = metrics.kid_from_features(features(real, det, dev, a.batch), features(fake, det, dev, a.batch, 256))
        print(f'kid {results["kid"]:.8f}  ({len(real)} real, {len(fake)} generated images, {a.detector})')
    if a.cmmd:
        det = metrics.ClipEmbeddingDetector(a.clip, dev)
        results['cmmd'] = metrics.cmmd_from_features(features(real, det, dev, a.batch), features(fake, det, dev, a.batch))
        print(f'cmmd {results["cmmd"]:.6f}  ({len(real)} real, {len(fake)} generated images, {a.clip})')
    return results


if __name__ == '__main__':
    main()
