#!/usr/bin/env python
"""Cost of the VAE encoder (sid_lsg_amd.vae.HipAutoencoderKLEncoder) and of its two new contraction kernels.
    python tools/vae_encode_cost.py encoder | attention | conv
One part per process, so that each runs under a time limit of its own (`timeout 300 python tools/vae_encode_cost.py attention`).
encoder    images/s of encode_latents at 512 x 512, batch 8, uint8 input, seeded `sd` weights
attention  ops.wide_attention (sidlsg_attn_fwd_wide) at (B 8, N 4096, D 512) and (B 4, N 9216, D 512) against
           torch.nn.functional.scaled_dot_product_attention on the same bf16 tensors, [B, 1, N, 512]
conv       the bottom/right-padded stride-2 conv (ops.conv3x3(pad='br')) against the existing stride-2 conv on an explicitly padded
           copy that yields the same outputs (`padded_equivalent`), at the three downsampler shapes of a 512 x 512 batch of 8
Device events around windows of back-to-back calls after warm-up, five windows per variant, the variants alternating; median and range.
Each line is printed and appended to profiles/vae_encoder.txt."""
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sid_lsg_amd import ops  # noqa: E402

dev = torch.device('cuda:0')
BF16 = torch.bfloat16
OUT = os.path.join(ROOT, 'profiles', 'vae_encoder.txt')


def say(line):
    print(line, flush=True)
    with open(OUT, 'a') as f:
        f.write(line + '\n')


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
        say(f'{title}: {name}: {statistics.median(v):.1f} us (median of 5 windows of {calls} calls, alternating; range {min(v):.1f} .. {max(v):.1f})')
    return {name: statistics.median(v) for name, v in samples.items()}


def padded_equivalent(x):
    """A copy on which the existing symmetric stride-2 conv computes the bottom/right-padded one: its output (i + 1, j + 1) reads rows
    2i + 1 .. 2i + 3 of its input, the new conv's output (i, j) rows 2i .. 2i + 2 of x, so the copy is x with a frame of zeros,
    [B, H + 2, W + 2, C], and outputs [1 : H/2 + 1, 1 : W/2 + 1] of the result are the wanted ones (row and column 0 are extra work)."""
    B, H, W, C = x.shape
    y = torch.zeros((B, H + 2, W + 2, C), device=x.device, dtype=x.dtype)
    y[:, 1:H + 1, 1:W + 1] = x
    return y


def main(part):
    say(f'--- vae_encode_cost.py {part}: {torch.cuda.get_device_name(0)}')
    g = torch.Generator().manual_seed(0)
    if part == 'encoder':
        from sid_lsg_amd.vae import HipAutoencoderKLEncoder
        B, R = 8, 512
        enc = HipAutoencoderKLEncoder('sd').init_parameters(0).to(dev)
        images = torch.randint(0, 256, (B, R, R, 3), generator=g, dtype=torch.uint8).to(dev)
        with torch.no_grad():
            enc.encode_latents(images)
            torch.cuda.synchronize()
            v = [window_us(lambda: enc.encode_latents(images), 3) for _ in range(5)]
        med = statistics.median(v)
        say(f'HipAutoencoderKLEncoder.encode_latents, sd weights (seeded), batch {B} at {R} x {R} uint8: {B / med * 1e6:.1f} images/s '
            f'({med / 1e3:.1f} ms per batch; median of 5 windows of 3 calls, range {min(v) / 1e3:.1f} .. {max(v) / 1e3:.1f} ms)')
    elif part == 'attention':
        for B, N in ((8, 4096), (4, 9216)):
            q, k, v = (torch.randn(B, N, 512, generator=g).to(dev, BF16) for _ in range(3))
            q4, k4, v4 = (t.view(B, 1, N, 512) for t in (q, k, v))
            with torch.no_grad():
                d = float((ops.wide_attention(q, k, v).float() - F.scaled_dot_product_attention(q4, k4, v4).view(B, N, 512).float()).abs().max())
            say(f'B {B}, N {N}, D 512: max |wide_attention - SDPA| (bf16 outputs) {d:.3e}')
            m = compare(f'one head of width 512, B {B}, N {N}, bf16', (('ops.wide_attention', lambda: ops.wide_attention(q, k, v)),
                                                                       ('torch SDPA', lambda: F.scaled_dot_product_attention(q4, k4, v4))), calls=5, warm=2)
            flop = 4.0 * B * N * N * 512
            say(f'B {B}, N {N}: wide_attention {flop / m["ops.wide_attention"] / 1e6:.1f} TFLOP/s, SDPA {flop / m["torch SDPA"] / 1e6:.1f} TFLOP/s')
    elif part == 'conv':
        for B, H, C in ((8, 512, 128), (8, 256, 256), (8, 128, 512)):
            x = torch.randn(B, H, H, C, generator=g).to(dev, BF16)
            w = (torch.randn(C, 9 * C, generator=g) * (9 * C) ** -0.5).to(dev, BF16)
            bias = torch.randn(C, generator=g).to(dev)
            xp = padded_equivalent(x)
            with torch.no_grad():
                a = ops.conv3x3(x, w, bias=bias, stride=2, pad='br')
                b = ops.conv3x3(xp, w, bias=bias, stride=2)[:, 1:H // 2 + 1, 1:H // 2 + 1]
            say(f'B {B}, {H} x {H}, C {C}: max |br conv - padded-copy conv| {float((a.float() - b.float()).abs().max()):.3e}')
            compare(f'stride-2 conv3x3, B {B}, {H} x {H}, C {C} -> {C}, bf16',
                    (("ops.conv3x3(pad='br')", lambda: ops.conv3x3(x, w, bias=bias, stride=2, pad='br')),
                     ('existing stride-2 conv on the padded copy (copy not timed)', lambda: ops.conv3x3(xp, w, bias=bias, stride=2)),
                     ('the same with the copy timed', lambda: ops.conv3x3(padded_equivalent(x), w, bias=bias, stride=2))), calls=10)
    else:
        raise SystemExit(__doc__)


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else '')
