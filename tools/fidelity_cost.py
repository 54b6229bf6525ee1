#!/usr/bin/env python
"""Cost of the paired fidelity metrics (sid_lsg_amd.fidelity) at B 8, 512 x 512:
  * sidlsg_psnr_ssim_u8 (one pass, fixed-order fp64 sums) against a torch chain of the same arithmetic on the device: the squared
    error, five fp64 depthwise 11 x 11 convolutions (x, y, x^2, y^2, xy) and the SSIM formula;
  * sidlsg_lpips_layer_f32 at the five tap shapes of VGG16 against the torch lines it replaces (normalise both halves, subtract,
    square, weight, mean);
  * a full LPIPS-VGG pass in pairs / s, with its multiply-accumulate count.
    python tools/fidelity_cost.py [batch=8] [side=512]
    python tools/fidelity_cost.py --diversity [side=512] [group=8]
--diversity measures the all-pairs form instead (sid_lsg_amd.diversity; profiles/diversity.txt keeps a run): sidlsg_lpips_group_f32 on
K maps against the paired launch on the gathered pair list at the five tap shapes, and HipLPIPS.group_pairs against HipLPIPS on the
pair list of one group.
Seeded inputs and weights.  Device events around windows of back-to-back calls after warm-up, five windows per variant, the variants
alternating; median and range.  Nothing is asserted on the times (profiles/fidelity.txt keeps a run)."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sid_lsg_amd import fidelity  # noqa: E402


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


def report(variants):
    samples = alternate(variants)
    for name, v in samples.items():
        print(line(name, v), flush=True)
    return [statistics.median(samples[n]) for n, _, _ in variants]


def torch_psnr_ssim(a, b, win2d):
    """The arithmetic of sidlsg_psnr_ssim_u8 in torch on the device -> (sse [B], ssim_sum [B])."""
    x, y = a.double(), b.double()
    sse = ((x - y) ** 2).sum(dim=(1, 2, 3))
    conv = lambda t: torch.nn.functional.conv2d(t, win2d, groups=3)  # noqa: E731
    mx, my = conv(x), conv(y)
    vx, vy, cxy = conv(x * x) - mx * mx, conv(y * y) - my * my, conv(x * y) - mx * my
    c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    ssim = ((2 * mx * my + c1) * (2 * cxy + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2))
    return sse, ssim.sum(dim=(1, 2, 3))


def torch_lpips_layer(F, w):
    B = F.shape[0] // 2
    n = F / (F.pow(2).sum(-1, keepdim=True).sqrt() + 1e-10)
    return (w * (n[:B] - n[B:]) ** 2).sum(-1).double().mean(dim=(1, 2))


def vgg_macs(H, W):
    """Multiply-accumulates of the 13 convolutions for ONE image (3 real input channels)."""
    total, h, w = 0, H, W
    for step in fidelity.VGG_LAYERS:
        if step == 'M':
            h, w = h // 2, w // 2
        elif step != 'T':
            total += h * w * 9 * step[1] * step[2]
    return total


def main(batch=8, side=512):
    dev = torch.device('cuda:0')
    print(f'device: {torch.cuda.get_device_name(0)}; {batch} pairs of {side} x {side}', flush=True)
    g = torch.Generator().manual_seed(0)
    a = torch.randint(0, 256, (batch, 3, side, side), generator=g, dtype=torch.uint8)
    b = (a.int() + torch.randint(-12, 13, a.shape, generator=g)).clamp(0, 255).to(torch.uint8)
    a, b = a.to(dev), b.to(dev)
    with torch.no_grad():
        x = torch.arange(-5, 6, dtype=torch.float64)
        w1 = torch.exp(-(x * x) / (2 * 1.5 * 1.5))
        w1 = w1 / w1.sum()
        win2d = (w1[:, None] * w1[None, :])[None, None].repeat(3, 1, 1, 1).to(dev)
        sums = fidelity.psnr_ssim_sums(a, b)
        variants = [('psnr_ssim   one pass', lambda: fidelity.psnr_ssim_sums(a, b), 200)]
        try:
            sse, ss = torch_psnr_ssim(a, b, win2d)
            print(f'    sse equal: {bool((sse == sums[:, 0]).all())}; max |ssim_sum - torch chain| / ssim_n {float(((ss - sums[:, 2]).abs() / sums[:, 3]).max()):.3g}', flush=True)
            variants.append(('psnr_ssim   torch chain', lambda: torch_psnr_ssim(a, b, win2d), 10))
        except Exception as e:          # a torch build without an fp64 depthwise convolution on the device
            print(f'    torch chain not available: {type(e).__name__}: {e}', flush=True)
        t = report(variants)
        if len(t) == 2:
            print(f'    one pass / torch chain {t[0] / t[1]:.3f}', flush=True)
        h = side
        for C in fidelity.TAP_CHANNELS:
            F = torch.relu(torch.randn(2 * batch, h, h, C, generator=g)).to(dev)
            w = torch.rand(C, generator=g).to(dev) / C
            err = float((fidelity.lpips_layer_f32(F, w) - torch_lpips_layer(F, w)).abs().max())
            t = report([(f'lpips_layer one launch  C {C:3d} {h:3d} x {h:3d}', lambda: fidelity.lpips_layer_f32(F, w), 50),
                        (f'lpips_layer torch lines C {C:3d} {h:3d} x {h:3d}', lambda: torch_lpips_layer(F, w), 10)])
            print(f'    one launch / torch lines {t[0] / t[1]:.3f}; max |one launch - torch lines| {err:.3g}', flush=True)
            del F
            h //= 2
        net = fidelity.HipLPIPS(*fidelity.random_state_dicts(0), dev)
        macs = 2 * vgg_macs(side, side)
        v = alternate([('pass', lambda: net(a, b), 2)])['pass']
        print(line(f'LPIPS-VGG pass, {batch} pairs', v, 'ms', 1.0), flush=True)
        ms = statistics.median(v)
        print(f'    {batch / ms * 1e3:.1f} pairs / s; {macs / 1e9:.1f} G multiply-accumulates per pair (two images, 13 convolutions), '
              f'{2 * macs * batch / ms / 1e9:.1f} TFLOP/s fp32', flush=True)


def diversity(side=512, group=8):
    """--diversity: (a) sidlsg_lpips_group_f32 on K maps against sidlsg_lpips_layer_f32 on the gathered list of their K (K - 1) / 2
    pairs (the gather itself is not timed), at the five tap shapes, K = 4, 8, 16; (b) HipLPIPS.group_pairs on one group against
    HipLPIPS.__call__ on its pair list."""
    from sid_lsg_amd import diversity as div
    dev = torch.device('cuda:0')
    print(f'device: {torch.cuda.get_device_name(0)}; all pairs of K maps, taps of {side} x {side}', flush=True)
    g, gd = torch.Generator().manual_seed(0), torch.Generator(dev).manual_seed(0)
    with torch.no_grad():
        h = side
        for C in fidelity.TAP_CHANNELS:
            w = torch.rand(C, generator=g).to(dev) / C
            for K in (4, 8, 16):
                table = div.pair_index(K).to(dev)
                step = min(table.shape[0], (fidelity.LIMIT - 1) // (2 * h * h * C * 4))      # pairs per paired launch: an operand stays below 2^31 bytes
                F = torch.relu(torch.randn(K, h, h, C, generator=gd, device=dev))
                lists = [torch.cat([F[table[s:s + step, 0]], F[table[s:s + step, 1]]]) for s in range(0, table.shape[0], step)]
                paired = lambda: torch.cat([fidelity.lpips_layer_f32(p, w) for p in lists])  # noqa: E731
                want = paired()
                fits = K * (K - 1) // 2 * 128 + 2048 * K * ((C + 63) // 64) <= 65536           # the on-chip form's admitted set (sidlsg_hip.h)
                forms = [('pairs on chip  ', 'chip')] * fits + [('pairs over grid', 'pairs')]
                same = all(torch.equal(fidelity.lpips_group_f32(F, w, K, form=form).reshape(-1), want) for form in [f for _, f in forms] + [None])
                t = report([(f'lpips_group on K maps, {name}   C {C:3d} {h:3d} x {h:3d} K {K:2d}', lambda form=form: fidelity.lpips_group_f32(F, w, K, form=form), 10)
                            for name, form in forms]
                           + [(f'lpips_layer, {len(lists):2d} launch(es) on the pairs  C {C:3d} {h:3d} x {h:3d} K {K:2d}', paired, 10)])
                pick = 'on chip' if fits and (h * h + 127) // 128 >= 512 else 'over grid'
                chip = f'on chip / paired {t[0] / t[-1]:.3f}' if fits else 'on chip: the copy of K vectors does not fit in LDS'
                print(f'    {chip}; over grid / paired {t[-2] / t[-1]:.3f}; the library takes "{pick}" here; bit-equal: {same}', flush=True)
                del F, lists
            h //= 2
        net = fidelity.HipLPIPS(*fidelity.random_state_dicts(0), dev)
        x = torch.randint(0, 256, (group, 3, side, side), generator=g, dtype=torch.uint8).to(dev)
        table = div.pair_index(group).to(dev)
        a, b = x[table[:, 0]].contiguous(), x[table[:, 1]].contiguous()
        same = torch.equal(net.group_pairs(x, group).reshape(-1), net(a, b))
        t = report_ms([(f'group_pairs, one group of {group}', lambda: net.group_pairs(x, group), 1),
                       (f'HipLPIPS on its {table.shape[0]} pairs', lambda: net(a, b), 1)])
        print(f'    group_pairs / pair list {t[0] / t[1]:.3f} ({t[1] / t[0]:.2f} x; the multiply-accumulate counts give {group - 1} x); bit-equal: {same}', flush=True)


def report_ms(variants):
    samples = alternate(variants)
    for name, v in samples.items():
        print(line(name, v, 'ms', 1.0), flush=True)
    return [statistics.median(samples[n]) for n, _, _ in variants]


if __name__ == '__main__':
    args = sys.argv[1:]
    if args and args[0] == '--diversity':
        diversity(int(args[1]) if len(args) > 1 else 512, int(args[2]) if len(args) > 2 else 8)
    else:
        main(int(args[0]) if args else 8, int(args[1]) if len(args) > 1 else 512)
