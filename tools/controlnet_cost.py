#!/usr/bin/env python
"""Cost of ControlNet conditioning (sid_lsg_amd.controlnet) at SD1.5 size: a UNet pass without control, the same pass with a control state,
and the one-off HipControlNet.prepare, next to the ratio the MAC counts predict.
    python tools/controlnet_cost.py [arch=sd15] [batch=8] [latent=64]
Seeded weights, batch 8 with guidance (16 rows of latent x latent latents, 8 control images of 8 latent x 8 latent), bf16.  Device events
around windows of back-to-back calls after warm-up, five windows per variant, the variants alternating; median and range.  Nothing is
asserted on the times (profiles/controlnet.txt keeps a run)."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sid_lsg_amd.controlnet import HipControlNet, controlnet_forward_macs  # noqa: E402
from sid_lsg_amd.unet import CONFIGS, HipUNet2DCondition, unet_forward_macs  # noqa: E402


def predicted_ratio(arch, h, w):
    """(UNet + ControlNet) / UNet multiply-accumulates of one pass: what the controlled pass should cost if both run at one rate."""
    u = unet_forward_macs(CONFIGS[arch], h, w)
    c, _ = controlnet_forward_macs(CONFIGS[arch], h, w)
    return (u + c) / u


def window_ms(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def main(arch='sd15', batch=8, lat=64):
    dev = torch.device('cuda:0')
    cfg = CONFIGS[arch]
    print(f'device: {torch.cuda.get_device_name(0)}; {arch}, batch {batch} with guidance ({2 * batch} rows), {lat} x {lat} latents, bf16', flush=True)
    u = unet_forward_macs(cfg, lat, lat)
    c, p = controlnet_forward_macs(cfg, lat, lat)
    print(f'MACs per row: UNet {u / 1e9:.1f} G, ControlNet {c / 1e9:.1f} G, prepare (per image) {p / 1e9:.2f} G; predicted ratio '
          f'controlled / plain {predicted_ratio(arch, lat, lat):.3f}', flush=True)
    unet = HipUNet2DCondition(cfg).materialize(dev, seed=0, with_grad_buffers=False).requires_grad_(False)
    net = HipControlNet(cfg).materialize(dev, seed=1)
    g = torch.Generator().manual_seed(0)
    n = 2 * batch
    x = torch.zeros(n, lat, lat, 8, dtype=torch.bfloat16)
    x[..., :4] = torch.randn(n, lat, lat, 4, generator=g).to(torch.bfloat16)
    x = x.to(dev)
    t = torch.full((n,), 500, dtype=torch.long, device=dev)
    ctx = torch.randn(n, cfg.text_len, cfg.cross_attention_dim, generator=g).to(dev, torch.bfloat16)
    images = torch.randint(0, 256, (batch, 8 * lat, 8 * lat, 3), generator=g, dtype=torch.uint8).to(dev)
    with torch.no_grad():
        state = net.prepare(images, 1.0, dup=2)
        variants = (('UNet pass', lambda: unet.forward_nhwc(x, t, ctx), 5), ('UNet pass with control', lambda: unet.forward_nhwc(x, t, ctx, control=state), 5),
                    ('prepare (once per batch)', lambda: net.prepare(images, 1.0, dup=2), 5))
        for _, fn, _ in variants:
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        samples = {name: [] for name, _, _ in variants}
        for _ in range(5):
            for name, fn, calls in variants:
                samples[name].append(window_ms(fn, calls))
    for name, v in samples.items():
        print(f'{name}: {statistics.median(v):.2f} ms (median of 5 windows, alternating; range {min(v):.2f} .. {max(v):.2f})', flush=True)
    print(f'measured ratio controlled / plain: {statistics.median(samples["UNet pass with control"]) / statistics.median(samples["UNet pass"]):.3f}', flush=True)


if __name__ == '__main__':
    a = sys.argv[1:]
    main(a[0] if a else 'sd15', int(a[1]) if len(a) > 1 else 8, int(a[2]) if len(a) > 2 else 64)
