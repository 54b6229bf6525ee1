#!/usr/bin/env python
"""Cost of the HPSv2 preprocessing kernel against a torch chain of the same transform, and of the scorer.
    python tools/hps_cost.py patches | detector
One part per process, so that each runs under a time limit of its own (`timeout 300 python tools/hps_cost.py patches`).  Batch 64 from
512 x 512 uint8 images.
patches   ops.pil_patches (224, patch 14, bf16) against the same arithmetic in torch: Pillow's two 8-bit passes as two fp64 GEMMs with the
          22-bit integer banks (exact, as metrics.resize_for_detector does for LANCZOS), `/ 255`, normalise, unfold, zero class row and
          pad, cast.  The two are compared bit for bit before they are timed.
detector  images/s of hps.score through load_clip('random:clip-vit-h-14', preprocess='pil'): the ViT-H/14 of HPSv2 with seeded weights
Device events around windows of back-to-back calls after warm-up, five windows per variant, the variants alternating; median and range."""
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sid_lsg_amd import hps, metrics, ops  # noqa: E402
from sid_lsg_amd.clip import load_clip  # noqa: E402

dev = torch.device('cuda:0')
BF16 = torch.bfloat16
B, SRC, R, P = 64, 512, 224, 14


def window_us(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / calls


def compare(title, variants, calls=20, warm=3):
    with torch.no_grad():
        for _, fn in variants:
            for _ in range(warm):
                fn()
        torch.cuda.synchronize()
        samples = {name: [] for name, _ in variants}
        for _ in range(5):
            for name, fn in variants:
                samples[name].append(window_us(fn, calls))
    for name, v in samples.items():
        print(f'{title}: {name}: {statistics.median(v):.1f} us (median of 5 windows of {calls} calls, alternating; range {min(v):.1f} .. {max(v):.1f})',
              flush=True)


def dense_bank(bounds, coeffs, n_in):
    """(bounds, coefficients) of one pass -> the [out, in] fp64 matrix of the same integers."""
    K = np.zeros((len(bounds), n_in), dtype=np.float64)
    for x, (x0, n) in enumerate(bounds):
        K[x, x0:x0 + n] = coeffs[x, :n]
    return torch.from_numpy(K).to(dev)


def main(part):
    print(f'device: {torch.cuda.get_device_name(0)}', flush=True)
    g = torch.Generator().manual_seed(0)
    images = torch.randint(0, 256, (B, 3, SRC, SRC), generator=g, dtype=torch.uint8).to(dev)
    if part == 'patches':
        plan = metrics.pil_crop_plan(SRC, SRC, R, P)
        kh, kv = dense_bank(plan['hbounds'], plan['hcoef'], SRC), dense_bank(plan['vbounds'], plan['vcoef'], SRC)
        mean, std = (torch.tensor(c, device=dev).view(1, 3, 1, 1) for c in (ops.CLIP_MEAN, ops.CLIP_STD))
        half, one, kp = float(1 << 21), float(1 << 22), ops.clip_patch_width(P)

        def chain():
            t = torch.matmul(images.to(torch.float64), kh.t())
            t = torch.floor((t + half) / one).clamp_(0, 255)
            t = torch.matmul(kv, t)
            t = torch.floor((t + half) / one).clamp_(0, 255).to(torch.float32)
            rows = F.unfold((t / 255. - mean) / std, P, stride=P).transpose(1, 2)
            return F.pad(rows, (0, kp - rows.shape[2], 1, 0)).to(BF16).reshape(-1, kp)
        got, want = ops.pil_patches(images, R, P), chain()
        print(f'elements that differ between the kernel and the torch chain (bf16 outputs): {int((got != want).sum())} of {got.numel()}', flush=True)
        compare(f'pil_patches, batch {B}, {SRC} x {SRC} -> {R}, patch {P}, bf16',
                (('ops.pil_patches (1 launch)', lambda: ops.pil_patches(images, R, P)), ('torch chain (2 fp64 GEMMs)', chain)))
    elif part == 'detector':
        det = load_clip('random:clip-vit-h-14', dev, preprocess='pil')
        texts = [f'a photo of object number {i} on a table' for i in range(B)]
        with torch.no_grad():
            hps.score(det, images, texts)
            torch.cuda.synchronize()
            v = [window_us(lambda: hps.score(det, images, texts), 2) for _ in range(5)]
        med = statistics.median(v)
        print(f'hps.score, random:clip-vit-h-14, batch {B} from {SRC} x {SRC} uint8, pil preprocessing, bf16 image tower + fp32 torch text tower: '
              f'{B / med * 1e6:.0f} images/s ({med / 1e3:.1f} ms per batch; median of 5 windows of 2 calls, range {min(v) / 1e3:.1f} .. {max(v) / 1e3:.1f} ms)',
              flush=True)
    else:
        raise SystemExit(__doc__)


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else '')
