#!/usr/bin/env python
"""Cost of LoRA merging (sid_lsg_amd.lora) at SD1.5 size, seeded weights, `random:lora` over ALL targets of the UNet and the text encoder
at ranks 4, 32 and 128:
  * the ONE merge launch per network (ops.lora_merge, sidlsg_lora_merge_f32) against the per-layer torch chain it replaces --
    `w.copy_(base + ((up * coef) @ down).view_as(w))` on the diffusers-layout parameter views, i.e. with the 3 x 3 convolutions' permute and
    the copy into the master view -- both from a saved copy of the masters into the masters, the same factors on the device;
  * LoraSet.attach (save, upload, job tables, launch, refresh), LoraSet.set_scales (coefficients, launch, refresh) and
    refresh_compute_weights alone, end to end with a device synchronisation.
    python tools/lora_cost.py [arch=sd15] [ranks=4,32,128] [out=profiles/lora.txt]
Device events around windows of back-to-back calls after warm-up, five windows per variant, the variants alternating; median and range.
Nothing is asserted on the times; the lines are printed and written to `out` BELOW the line that starts with MARKER: whatever the
file holds above that line (profiles/lora.txt: the figures printed by tests/test_gpu_lora.py) is kept."""
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sid_lsg_amd import lora  # noqa: E402
from sid_lsg_amd.text import TEXT_CONFIGS, CLIPTextModel  # noqa: E402
from sid_lsg_amd.unet import CONFIGS, HipUNet2DCondition  # noqa: E402

LINES = []
MARKER = '== python tools/lora_cost.py'


def say(s):
    print(s, flush=True)
    LINES.append(s)


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
        fn()
    torch.cuda.synchronize()
    samples = {name: [] for name, _, _ in variants}
    for _ in range(windows):
        for name, fn, calls in variants:
            samples[name].append(window_ms(fn, calls))
    return samples


def line(name, v):
    return f'{name}: {statistics.median(v):.3f} ms (median of {len(v)} windows, alternating; range {min(v):.3f} .. {max(v):.3f})'


def wall_ms(fn, reps=3):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def torch_chain(unet, te, adapters, nets, scale):
    """The per-layer chain over the same saved base copies: [(parameter view, base in the view's shape, up [n, r], down [r, cin k k], coef [r])]."""
    mods = {'unet': dict(unet.named_modules()), 'te': dict(te.named_modules())}
    dev = unet.flat_params.device
    jobs = []
    for net in ('unet', 'te'):
        nm = nets[net]
        by_name = {L['layer'].name: (L, b) for L, b in zip(nm.plan.layers, nm.base_views)}
        for target, down, up, alpha, rank in adapters:
            if target[0] != net:
                continue
            L, b = by_name[target[1]]
            w = mods[net][target[1]].weight.data
            layer = L['layer']
            if layer.kind == 'conv3x3':
                base = b.view(layer.n, 3, 3, layer.cin).permute(0, 3, 1, 2)          # the master's physical layout seen in the parameter's shape
            else:
                base = b.view(w.shape)
            coef = torch.full((rank,), scale * alpha / rank, device=dev)
            jobs.append((w, base, up.reshape(layer.n, rank).to(dev), down.reshape(rank, -1).to(dev), coef))

    def run():
        for w, base, up, down, coef in jobs:
            w.copy_(base + ((up * coef) @ down).view_as(w))
    return run


def main(arch='sd15', ranks=(4, 32, 128), out=os.path.join(ROOT, 'profiles', 'lora.txt')):
    dev = torch.device('cuda:0')
    cfg = CONFIGS[arch]
    say(f'device: {torch.cuda.get_device_name(0)}; {arch}, random:lora over all targets, fp32 masters, bf16 compute copies')
    with torch.no_grad():
        unet = HipUNet2DCondition(cfg).materialize(dev, seed=0, with_grad_buffers=False).requires_grad_(False)
        torch.manual_seed(1)
        te = CLIPTextModel(max_pos=cfg.text_len, **TEXT_CONFIGS[arch]).requires_grad_(False).eval().to(dev)
        p0 = unet.flat_params.clone()
        say(line('refresh_compute_weights alone', wall_ms(unet.refresh_compute_weights, 5)).replace('windows, alternating', 'calls, wall clock'))
        for rank in ranks:
            sd = lora.random_lora_state_dict(unet, te, rank, seed=rank)
            ad = lora.parse_lora(sd, unet, te)
            del sd
            ls = lora.LoraSet(unet, te)
            t_attach = wall_ms(lambda: (ls.detach() if ls.attached else None, ls.attach([ad], [1.0])), 3)
            nets = ls._nets
            nu, nt = len(nets['unet'].plan.layers), len(nets['te'].plan.layers)
            elems = sum(L['layer'].n * L['layer'].kk for nm in nets.values() for L in nm.plan.layers)
            say(f'rank {rank}: {nu} UNet + {nt} text-encoder layers, {elems / 1e6:.1f} M master elements touched, '
                f'{nets["unet"].table.nblocks + nets["te"].table.nblocks} tiles; factors {(nets["unet"].up.numel() + nets["unet"].down.numel() + nets["te"].up.numel() + nets["te"].down.numel()) * 4 / 2 ** 20:.0f} MiB')
            merged = unet.flat_params.clone()
            chain = torch_chain(unet, te, ad, nets, 1.0)
            chain()
            err = float((unet.flat_params - merged).abs().max())

            def launch():
                for nm in nets.values():
                    lora.ops.lora_merge(nm.table)
            variants = ((f'rank {rank:3d} one merge launch per network', launch, 3), (f'rank {rank:3d} per-layer torch chain       ', chain, 3))
            samples = alternate(variants)
            for name, v in samples.items():
                say(line(name, v))
            a, b = (statistics.median(samples[n]) for n, _, _ in variants)
            say(f'    merge launches / torch chain {a / b:.3f}; {2 * 4 * elems / a / 1e6:.0f} GB/s of base read + dst written by the launches; '
                f'max |launch - chain| on the masters {err:.3g}')
            launch()
            assert torch.equal(unet.flat_params, merged)
            say(line(f'rank {rank:3d} LoraSet.attach, end to end (after detach)', t_attach).replace('windows, alternating', 'calls, wall clock, first included'))
            say(line(f'rank {rank:3d} LoraSet.set_scales, end to end', wall_ms(lambda: ls.set_scales([0.5]), 5)).replace('windows, alternating', 'calls, wall clock'))
            ls.detach()
            assert torch.equal(unet.flat_params, p0)
            del ls, nets, chain, merged, ad
            torch.cuda.empty_cache()
    write_section(out, LINES)


def write_section(out, lines):
    """Replace the tool's section of `out` (from the MARKER line to the end), keeping everything above it."""
    head = []
    if os.path.isfile(out):
        with open(out) as f:
            for ln in f.read().splitlines():
                if ln.startswith(MARKER):
                    break
                head.append(ln)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:
        f.write('\n'.join(head + [MARKER + ' (SD1.5 size, random:lora over all targets) =='] + list(lines)) + '\n')


if __name__ == '__main__':
    a = sys.argv[1:]
    main(a[0] if a else 'sd15', tuple(int(r) for r in a[1].split(',')) if len(a) > 1 else (4, 32, 128), a[2] if len(a) > 2 else os.path.join(ROOT, 'profiles', 'lora.txt'))
