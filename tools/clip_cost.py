#!/usr/bin/env python
"""Cost of the CLIP detector (sid_lsg_amd.clip) and of its two elementwise kernels against the torch chains they replace.
    python tools/clip_cost.py patches | gelu | detector:vit-l-14 | detector:vit-g-14
One part per process, so that each runs under a time limit of its own (`timeout 300 python tools/clip_cost.py gelu`).  Batch 64 from
256 x 256 uint8 images, seeded weights (load_clip('random:clip-<arch>')).
patches   ops.clip_patches (224, patch 14, bf16) against `/255`, F.interpolate(bicubic), normalise, unfold, zero class row and pad, cast
gelu      ops.gelu on the fc1 output shapes [64 * 257, 4096] (quick_gelu) and [64 * 257, 6144] (gelu), bf16, against x * sigmoid(1.702 x) / F.gelu
detector  images/s of HipCLIPDetector.scores, text side included
Device events around windows of back-to-back calls after warm-up, five windows per variant, the variants alternating; median and range."""
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sid_lsg_amd import ops  # noqa: E402
from sid_lsg_amd.clip import load_clip  # noqa: E402

dev = torch.device('cuda:0')
BF16 = torch.bfloat16
B, SRC, R, P = 64, 256, 224, 14


def window_us(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / calls


def compare(title, variants, calls=50, warm=5):
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


def main(part):
    print(f'device: {torch.cuda.get_device_name(0)}', flush=True)
    g = torch.Generator().manual_seed(0)
    images = torch.randint(0, 256, (B, 3, SRC, SRC), generator=g, dtype=torch.uint8).to(dev)
    if part == 'patches':
        mean, std = (torch.tensor(c, device=dev).view(1, 3, 1, 1) for c in (ops.CLIP_MEAN, ops.CLIP_STD))
        kp = ops.clip_patch_width(P)

        def chain():
            x = F.interpolate(images.to(torch.float32) / 255., R, mode='bicubic', align_corners=False)
            rows = F.unfold((x - mean) / std, P, stride=P).transpose(1, 2)                          # [B, 256, 588]
            return F.pad(rows, (0, kp - rows.shape[2], 1, 0)).to(BF16).reshape(-1, kp)
        got, want = ops.clip_patches(images, R, P), chain()
        print(f'max |kernel - torch chain| (bf16 outputs): {float((got.float() - want.float()).abs().max()):.3e}', flush=True)
        compare(f'clip_patches, batch {B}, {SRC} x {SRC} -> {R}, patch {P}, bf16',
                (('ops.clip_patches (1 launch)', lambda: ops.clip_patches(images, R, P)), ('torch chain', chain)))
    elif part == 'gelu':
        for mode, width in (('quick_gelu', 4096), ('gelu', 6144)):
            x = torch.randn(B * 257, width, generator=g).to(dev, BF16)
            torch_fn = (lambda: x * torch.sigmoid(1.702 * x)) if mode == 'quick_gelu' else (lambda: F.gelu(x))
            compare(f'{mode} on [{B * 257}, {width}] bf16 ({x.numel() * 4 / 1e6:.0f} MB moved)',
                    ((f'ops.gelu', lambda: ops.gelu(x, mode)), ('torch', torch_fn)))
    elif part.startswith('detector:'):
        det = load_clip('random:clip-' + part.split(':', 1)[1], dev)
        texts = [f'a photo of object number {i} on a table' for i in range(B)]
        with torch.no_grad():
            det.scores(images, texts)
            torch.cuda.synchronize()
            v = [window_us(lambda: det.scores(images, texts), 3) for _ in range(5)]
        med = statistics.median(v)
        print(f'HipCLIPDetector.scores, {part}, batch {B} from {SRC} x {SRC} uint8, bf16 image tower + fp32 torch text tower: '
              f'{B / med * 1e6:.0f} images/s ({med / 1e3:.1f} ms per batch; median of 5 windows of 3 calls, range {min(v) / 1e3:.1f} .. {max(v) / 1e3:.1f} ms)',
              flush=True)
    else:
        raise SystemExit(__doc__)


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else '')
