#!/usr/bin/env python
"""Cost of the Canny edge detector (sid_lsg_amd.edges) at B 8, 512 x 512 and 768 x 768:
  * sidlsg_canny_classify_u8 (one launch) against a torch chain of the same integer arithmetic on the device (replicate pad, shifted
    slices for the Sobel, the channel choice by argmax, the three suppression cases by torch.where, two bit-packing sums);
  * sidlsg_edge_hysteresis (one launch, one workgroup per image) against a max_pool2d loop run for the SAME number of rounds the kernel
    reports, without the host check of "changed" a torch program would need to know when to stop (the rounds a plain dilation loop
    needs to finish, its geodesic depth, are printed next to it: the kernel's rounds fill runs inside a word, the loop's do not);
  * edges.canny end to end in images / s, and the hysteresis rounds it took;
  * at 512 x 512, the VAE decode of the same batch (seeded weights of the SD architecture) in the same session, and the rounds on its
    decoded sample.
    python tools/canny_cost.py [batch=8]
Inputs: the smoothed-noise recipe of the tests (Gaussian-filtered normal noise, sigma 2, scaled to 0 .. 255).  Device events around
windows of back-to-back calls after warm-up, five windows per variant, the variants alternating; median and range.  Nothing is asserted
on the times (profiles/canny.txt keeps a run)."""
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sid_lsg_amd import edges  # noqa: E402

TG22 = 13573


def window_ms(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def report(variants, windows=5, unit='us', k=1e3):
    for _, fn, _ in variants:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    samples = {name: [] for name, _, _ in variants}
    for _ in range(windows):
        for name, fn, calls in variants:
            samples[name].append(window_ms(fn, calls))
    d = 1 if unit == 'us' else 3
    for name, v in samples.items():
        print(f'{name}: {statistics.median(v) * k:.{d}f} {unit} (median of {len(v)} windows, alternating; range {min(v) * k:.{d}f} .. {max(v) * k:.{d}f})', flush=True)
    return [statistics.median(samples[n]) for n, _, _ in variants]


def smoothed_noise(B, H, W, sigma, seed):
    from scipy import ndimage
    out = []
    for i in range(B):
        f = ndimage.gaussian_filter(np.random.default_rng(seed + i).standard_normal((H, W, 3)), (sigma, sigma, 0))
        out.append(np.round((f - f.min()) / (f.max() - f.min()) * 255).astype(np.uint8))
    return np.stack(out)


def pack_words(mask):
    """bool [B, H, W] (W % 32 == 0) -> int32 [B, H, W / 32] on the device."""
    B, H, W = mask.shape
    w = (mask.reshape(B, H, W // 32, 32).long() << torch.arange(32, device=mask.device)).sum(-1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).int()


def torch_classify(img, low, high):
    """The arithmetic of sidlsg_canny_classify_u8 as a torch chain -> (cand, strong) bit planes."""
    x = img.permute(0, 3, 1, 2).float()
    p = torch.nn.functional.pad(x, (1, 1, 1, 1), mode='replicate').int()
    H, W = img.shape[1], img.shape[2]
    s = lambda dy, dx: p[:, :, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]  # noqa: E731
    gx = (s(-1, 1) + 2 * s(0, 1) + s(1, 1)) - (s(-1, -1) + 2 * s(0, -1) + s(1, -1))
    gy = (s(1, -1) + 2 * s(1, 0) + s(1, 1)) - (s(-1, -1) + 2 * s(-1, 0) + s(-1, 1))
    mag = gx.abs() + gy.abs()
    c = mag.argmax(dim=1, keepdim=True)                      # the first maximal channel
    dx, dy, m = gx.gather(1, c)[:, 0], gy.gather(1, c)[:, 0], mag.gather(1, c)[:, 0]
    mp = torch.nn.functional.pad(m, (1, 1, 1, 1))
    n = lambda dy_, dx_: mp[:, 1 + dy_:1 + dy_ + H, 1 + dx_:1 + dx_ + W]  # noqa: E731
    ax, ay = dx.abs(), dy.abs() << 15
    t22 = ax * TG22
    t67 = t22 + (ax << 16)
    horiz = (m > n(0, -1)) & (m >= n(0, 1))
    vert = (m > n(-1, 0)) & (m >= n(1, 0))
    neg = (dx ^ dy) < 0
    diag = torch.where(neg, (m > n(-1, 1)) & (m > n(1, -1)), (m > n(-1, -1)) & (m > n(1, 1)))
    keep = (m > low) & torch.where(ay < t22, horiz, torch.where(ay > t67, vert, diag))
    return pack_words(keep), pack_words(keep & (m > high))


def unpack_words(words, W):
    return ((words.long()[..., None] >> torch.arange(32, device=words.device)) & 1).reshape(words.shape[0], words.shape[1], -1)[..., :W].bool()


def torch_hysteresis(cand, strong, rounds):
    """`rounds` rounds of E = C & max_pool2d(E, 3, 1, 1) on half maps; no host check."""
    e = strong * cand
    for _ in range(rounds):
        e = cand * torch.nn.functional.max_pool2d(e, 3, 1, 1)
    return e


def geodesic_rounds(cand, strong):
    e, n = strong * cand, 0
    while True:
        g = cand * torch.nn.functional.max_pool2d(e, 3, 1, 1)
        if torch.equal(g, e):
            return n + 1, e
        e, n = g, n + 1


def one_size(batch, side, dev):
    print(f'-- {batch} images of {side} x {side} (smoothed noise, sigma 2) --', flush=True)
    img = torch.from_numpy(smoothed_noise(batch, side, side, 2.0, 100)).to(dev)
    cand, strong = edges.classify(img)
    tc, ts = torch_classify(img, 100, 200)
    print(f'    classify: the torch chain gives the same planes: {torch.equal(tc, cand) and torch.equal(ts, strong)}', flush=True)
    t = report([('classify    one launch ', lambda: edges.classify(img), 100), ('classify    torch chain', lambda: torch_classify(img, 100, 200), 10)])
    print(f'    one launch / torch chain {t[0] / t[1]:.3f}', flush=True)
    e, _, rounds = edges.hysteresis(cand, strong, side, side)
    r = int(rounds.max())
    ch, sh = unpack_words(cand, side).half()[:, None], unpack_words(strong, side).half()[:, None]
    need, fixed = geodesic_rounds(ch, sh)
    same = torch.equal(fixed[:, 0].bool(), unpack_words(e, side))
    print(f'    hysteresis: rounds per image {rounds.tolist()}; a plain dilation loop needs {need} rounds for the batch; same edges: {same}', flush=True)
    t = report([('hysteresis  one launch ', lambda: edges.hysteresis(cand, strong, side, side), 50),
                (f'hysteresis  max_pool2d x {r}', lambda: torch_hysteresis(ch, sh, r), 5)])
    print(f'    one launch / max_pool2d loop of {r} rounds {t[0] / t[1]:.3f}', flush=True)
    t = report([('canny       end to end ', lambda: edges.canny(img), 50)], unit='ms', k=1.0)
    print(f'    {batch / t[0] * 1e3:.0f} images / s; {int(unpack_words(e, side).sum())} edge pixels in the batch', flush=True)
    return t[0]


def main(batch=8):
    dev = torch.device('cuda:0')
    print(f'device: {torch.cuda.get_device_name(0)}', flush=True)
    with torch.no_grad():
        canny_ms = one_size(batch, 512, dev)
        from sid_lsg_amd.vae import HipAutoencoderKLDecoder
        vae = HipAutoencoderKLDecoder('sd').init_parameters(2).to(dev)
        z = torch.randn(batch, 4, 64, 64, generator=torch.Generator().manual_seed(0)).to(dev)
        sample = (vae.decode(z)[0] * 127.5 + 128).clip(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
        maps = edges.canny(sample)
        print(f'-- VAE decode of {batch} latents to 512 x 512 (seeded weights of the SD architecture) --', flush=True)
        print(f'    canny on the decoded sample: rounds per image {maps.rounds.tolist()}, {int(maps.to_bool().sum())} edge pixels', flush=True)
        t = report([('vae decode ', lambda: vae.decode(z), 2), ('canny on the decoded sample', lambda: edges.canny(sample), 20)], unit='ms', k=1.0)
        print(f'    canny / decode {t[1] / t[0]:.4f} on the decoded sample, {canny_ms / t[0]:.4f} on the smoothed noise', flush=True)
        one_size(batch, 768, dev)


if __name__ == '__main__':
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 8)
