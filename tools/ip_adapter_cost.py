#!/usr/bin/env python
"""Cost of IP-Adapter image prompts (sid_lsg_amd.ip_adapter) at SD1.5 size:
  * the ONE launch of the decoupled cross-attention (ops.cross_attention2, sidlsg_attn_cross2_fwd_ps) against the chain it replaces,
    built from the entry points that existed before it -- attn_fwd over the text keys, attn_fwd over the image keys, one scaled add
    (torch's `add_(o2, alpha=s)`) -- at SD1.5's four cross-attention shapes, B 16, H 8, Nk 77, Nk2 4; the text attention alone
    (ops.cross_attention) is timed next to them as the floor;
  * HipIPAdapter.prepare (once per batch);
  * a full UNet pass with and without an image-prompt state.
    python tools/ip_adapter_cost.py [arch=sd15] [batch=8] [latent=64]
Seeded weights, batch 8 with guidance (16 rows), bf16.  Device events around windows of back-to-back calls after warm-up, five windows
per variant, the variants alternating; median and range.  Nothing is asserted on the times (profiles/ip_adapter.txt keeps a run)."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sid_lsg_amd import ops  # noqa: E402
from sid_lsg_amd.ip_adapter import HipIPAdapter, random_state_dict  # noqa: E402
from sid_lsg_amd.unet import CONFIGS, HipUNet2DCondition  # noqa: E402

SHAPES = ((4096, 40), (1024, 80), (256, 160), (64, 160))       # (Nq, D) of SD1.5's cross-attention layers at 64 x 64 latents
LOG2E = 1.4426950408889634


def window_ms(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def alternate(variants, windows=5):
    for _, fn, _ in variants:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    samples = {name: [] for name, _, _ in variants}
    for _ in range(windows):
        for name, fn, calls in variants:
            samples[name].append(window_ms(fn, calls))
    return samples


def line(name, v, unit='us', k=1e3):
    d = 1 if unit == 'us' else 2
    return f'{name}: {statistics.median(v) * k:.{d}f} {unit} (median of {len(v)} windows, alternating; range {min(v) * k:.{d}f} .. {max(v) * k:.{d}f})'


def kernel_rows(dev, B=16, H=8, Nk=77, Nk2=4, s=0.7):
    g = torch.Generator().manual_seed(0)
    for Nq, D in SHAPES:
        C = H * D
        q = (torch.randn(B, Nq, C, generator=g) * (D ** -0.5 * LOG2E)).to(dev, torch.bfloat16)      # pre-scaled, as the bf16 UNet's queries are
        kv = torch.randn(B, Nk, 2 * C, generator=g).to(dev, torch.bfloat16)
        wide = torch.randn(B, Nk2, 24960, generator=g).to(dev, torch.bfloat16)                      # SD1.5's sum 2 C_l columns
        view = wide[:, :, 1280:1280 + 2 * C]
        tight = view.contiguous()

        def chain():
            o = ops.cross_attention(q, kv, H, True)
            return o.add_(ops.cross_attention(q, tight, H, True), alpha=s)

        variants = ((f'one launch  Nq {Nq:4d} D {D:3d}', lambda: ops.cross_attention2(q, kv, view, H, s, True), 500),
                    (f'chain of 3  Nq {Nq:4d} D {D:3d}', chain, 500),
                    (f'text only   Nq {Nq:4d} D {D:3d}', lambda: ops.cross_attention(q, kv, H, True), 500))
        err = float((variants[0][1]().float() - chain().float()).abs().max())
        samples = alternate(variants)
        for name, v in samples.items():
            print(line(name, v), flush=True)
        one, three, text = (statistics.median(samples[n]) for n, _, _ in variants)
        print(f'    one launch / chain {one / three:.3f}, one launch / text only {one / text:.3f}; max |one launch - chain| {err:.3g}', flush=True)


def main(arch='sd15', batch=8, lat=64):
    dev = torch.device('cuda:0')
    cfg = CONFIGS[arch]
    print(f'device: {torch.cuda.get_device_name(0)}; {arch}, batch {batch} with guidance ({2 * batch} rows), {lat} x {lat} latents, bf16', flush=True)
    with torch.no_grad():
        kernel_rows(dev)
        unet = HipUNet2DCondition(cfg).materialize(dev, seed=0, with_grad_buffers=False).requires_grad_(False)
        E = 1024 if cfg.cross_attention_dim == 1024 else 768
        ad = HipIPAdapter(cfg, random_state_dict(cfg, E, seed=1), dev, torch.bfloat16, E)
        g = torch.Generator().manual_seed(0)
        n = 2 * batch
        x = torch.zeros(n, lat, lat, 8, dtype=torch.bfloat16)
        x[..., :4] = torch.randn(n, lat, lat, 4, generator=g).to(torch.bfloat16)
        x = x.to(dev)
        t = torch.full((n,), 500, dtype=torch.long, device=dev)
        ctx = torch.randn(n, cfg.text_len, cfg.cross_attention_dim, generator=g).to(dev, torch.bfloat16)
        emb = torch.randn(batch, E, generator=g).to(dev)
        state = ad.prepare(emb, 1.0, dup=2)
        variants = (('UNet pass', lambda: unet.forward_nhwc(x, t, ctx), 10), ('UNet pass with image prompt', lambda: unet.forward_nhwc(x, t, ctx, ip=state), 10),
                    ('prepare (once per batch)', lambda: ad.prepare(emb, 1.0, dup=2), 100))
        samples = alternate(variants)
    for name, v in samples.items():
        print(line(name, v) if name.startswith('prepare') else line(name, v, 'ms', 1.0), flush=True)
    print(f'measured ratio image-prompted / plain: {statistics.median(samples["UNet pass with image prompt"]) / statistics.median(samples["UNet pass"]):.4f}', flush=True)


if __name__ == '__main__':
    a = sys.argv[1:]
    main(a[0] if a else 'sd15', int(a[1]) if len(a) > 1 else 8, int(a[2]) if len(a) > 2 else 64)
