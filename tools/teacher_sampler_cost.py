#!/usr/bin/env python
"""Cost of sampling the teacher (sd_util.teacher_sample) and of its step-boundary kernel.
    python tools/teacher_sampler_cost.py
(a) sidlsg_ddim_step against the three launches it replaces (cfg_x0 mode 1, cfg_x0 mode 0, noisy_input) at B = 8, 64 x 64 latents,
    [uncond ; cond] input, bf16 activations: device events around windows of 200 back-to-back calls after 20 warm-up calls, five
    windows per variant, the two variants alternating; the median and the range.  Back-to-back launches of a ~4 MB kernel measure
    launch throughput as much as the kernel, which is what the sampler loop sees.
(b) images/s of teacher_sample at SD1.5 size with seeded weights (random:sd15), 50 steps, kappa = 7.5, batch 8, 512 x 512, with and
    without the VAE decode: host clock around a call that ends in torch.cuda.synchronize, one warm-up call, three timed calls.
    python tools/teacher_sampler_cost.py --solver
the solver family of sd_util.teacher_sample_solver instead, measured the same two ways:
(c) sidlsg_solver_step on a second-order DPM-Solver++ 2M row, alone and behind a sidlsg_cfg_rescale_stats launch, against
    sidlsg_ddim_step and against a chain of torch operations with the same arithmetic (guided combine, x0, three-term update, NHWC
    input of both halves), the four variants alternating;
(d) images/s of teacher_sample_solver with 'dpmpp2m' at 20 steps against teacher_sample ('ddim') at 50, both without the VAE decode.
    python tools/teacher_sampler_cost.py --masked
the masked step boundary of inpainting (sd_util.teacher_sample_solver_i2i with a mask):
(e) sidlsg_masked_renoise as the one new launch against the chain of existing launches that does the same job (noisy_input for the
    known region, torch.where, noisy_input for the next input), measured as (a), the two variants alternating;
(f) images/s of 'dpmpp2m' at 20 steps with and without a mask (image-to-image at start_index 0, half of the latent repainted),
    without the VAE decode."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sid_lsg_amd import ops  # noqa: E402
from sid_lsg_amd.scheduler import DDPMScheduler  # noqa: E402
from sid_lsg_amd.sd_util import load_sd15, teacher_sample, teacher_sample_solver, teacher_sample_solver_i2i  # noqa: E402

args = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
args.add_argument('--solver', action='store_true', help='measure sidlsg_solver_step and teacher_sample_solver (sections c and d) instead of a and b')
args.add_argument('--masked', action='store_true', help='measure sidlsg_masked_renoise and the masked dpmpp2m sampler (sections e and f) instead')
args = args.parse_args()
dev = torch.device('cuda:0')
BF16 = torch.bfloat16
print(f'device: {torch.cuda.get_device_name(0)}', flush=True)

# ---- (a) the step-boundary kernel ----
B, lat, kappa = 8, 64, 7.5
g = torch.Generator().manual_seed(0)
eps = torch.randn(2 * B, lat * lat, 8, generator=g).to(dev)
xt = torch.randn(B, 4, lat, lat, generator=g).to(dev)
sched = DDPMScheduler().to(dev)
t = torch.full((B,), 501, dtype=torch.long, device=dev)
s0, s1 = sched.coefficients(t)
s0p, s1p = sched.coefficients(t - 20)


def fused():
    return ops.ddim_step(eps, xt, s0, s1, s0p, s1p, kappa, BF16)


def chain():
    x0 = ops.cfg_x0(eps, xt, s0, s1, kappa, True, BF16)
    e = ops.cfg_x0(eps, xt, s0, s1, kappa, False, BF16)
    return ops.noisy_input(x0, e, s0p, s1p, 2, BF16)


def window_us(fn, calls=200):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / calls


def alternate(variants, label):
    """Median and range of five windows per variant, the variants alternating inside one process."""
    with torch.no_grad():
        for _, fn in variants:
            for _ in range(20):
                fn()
        torch.cuda.synchronize()
        samples = {name: [] for name, _ in variants}
        for _ in range(5):
            for name, fn in variants:
                samples[name].append(window_us(fn))
    for name, v in samples.items():
        print(f'({label}) {name}: {statistics.median(v):.1f} us per step boundary (median of 5 windows of 200 back-to-back calls, alternating with '
              f'the other variants; range {min(v):.1f} .. {max(v):.1f}); B = {B}, {lat} x {lat} latents, dup 2, bf16', flush=True)


def solver_sections():
    coef = torch.tensor([[0.875, 0.4347, -0.116, 0.0]] * B, device=dev)          # a second-order 2M row
    x0p = torch.randn(B, 4, lat, lat, generator=g).to(dev)
    hist = torch.empty_like(xt)
    cx, cc, cp = (coef[:, j].view(B, 1, 1, 1).contiguous() for j in range(3))
    a0, a1 = s0.view(B, 1, 1, 1), s1.view(B, 1, 1, 1)

    def solver():
        return ops.solver_step(eps, xt, s0, s1, coef, kappa, BF16, x0p=x0p, x0_out=hist)

    def solver_rescaled():
        return ops.solver_step(eps, xt, s0, s1, coef, kappa, BF16, x0p=x0p, x0_out=hist, scale=ops.cfg_rescale_stats(eps, 4, kappa, 0.7))

    def torch_chain():
        u, c = eps[:B, :, :4], eps[B:, :, :4]
        e = (u + kappa * (c - u)).view(B, lat, lat, 4).permute(0, 3, 1, 2)
        x0 = (xt - a1 * e) / a0
        x = cx * xt + cc * x0 + cp * x0p
        nhwc = torch.zeros(2 * B, lat, lat, 8, device=dev, dtype=BF16)
        nhwc[:B, ..., :4] = nhwc[B:, ..., :4] = x.permute(0, 2, 3, 1).to(BF16)
        return nhwc, x, x0
    alternate((('solver_step (1 launch)', solver), ('cfg_rescale_stats + solver_step (2 launches)', solver_rescaled),
               ('ddim_step (1 launch)', fused), ('torch chain of the same arithmetic', torch_chain)), 'c')
    print(f'    solver_step reads and writes {(eps.numel() * 4 + 4 * xt.numel() * 4 + 2 * B * lat * lat * 8 * 2) / 1e6:.2f} MB per launch; '
          f'cfg_rescale_stats reads {eps.numel() * 4 / 1e6:.2f} MB twice', flush=True)
    res = 512
    unet, vae, sched, te, tok = load_sd15('random:sd15', None, dev, BF16)
    unet.eval().requires_grad_(False)
    prompts = [f'a photo of object number {i} on a table, studio light' for i in range(B)]
    z = torch.randn(B, 4, res // 8, res // 8, generator=g).to(dev)
    runs = (('teacher_sample_solver, dpmpp2m', 20, lambda: teacher_sample_solver(unet, z, prompts, sched, te, tok, res, guidance_scale=kappa,
                                                                                num_inference_steps=20, solver='dpmpp2m')),
            ('teacher_sample_solver, dpmpp2m, guidance rescale 0.7', 20,
             lambda: teacher_sample_solver(unet, z, prompts, sched, te, tok, res, guidance_scale=kappa, num_inference_steps=20, solver='dpmpp2m',
                                           guidance_rescale=0.7)),
            ('teacher_sample (ddim)', 50, lambda: teacher_sample(unet, z, prompts, sched, te, tok, res, guidance_scale=kappa, num_inference_steps=50)))
    for name, steps, fn in runs:
        times = []
        for rep in range(4):
            torch.cuda.synchronize()
            t0 = time.time()
            fn()
            torch.cuda.synchronize()
            if rep:
                times.append(time.time() - t0)
        med = statistics.median(times)
        print(f'(d) {name}, random:sd15, {res} x {res}, batch {B}, {steps} steps, kappa {kappa}, without VAE decode: {B / med:.2f} images/s '
              f'({med:.2f} s per batch, median of 3 after one warm-up call; {min(times):.2f} .. {max(times):.2f} s)', flush=True)


def masked_sections():
    z0 = torch.randn(B, 4, lat, lat, generator=g).to(dev)
    z = torch.randn(B, 4, lat, lat, generator=g).to(dev)
    mask = torch.zeros(B, lat, lat, dtype=torch.uint8, device=dev)
    mask[:, :, lat // 2:] = 1
    m4 = mask.bool()[:, None]
    ones = torch.ones(B, device=dev)

    def fused_mask():
        return ops.masked_renoise(xt, z0, mask, noise=z, a0=s0p, a1=s1p, dup=2, act_dtype=BF16)

    def chain_mask():
        xn = torch.where(m4, xt, ops.noisy_input(z0, z, s0p, s1p, 1, BF16)[1])
        return ops.noisy_input(None, xn, ones, ones, 2, BF16)[0], xn
    with torch.no_grad():
        a, b = fused_mask(), chain_mask()
        torch.cuda.synchronize()
        print(f'(e) the two variants agree bit for bit: {torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])}', flush=True)
    alternate((('masked_renoise (1 launch)', fused_mask), ('noisy_input + torch.where + noisy_input (3 launches)', chain_mask)), 'e')
    print(f'    masked_renoise reads and writes {(4 * xt.numel() * 4 + mask.numel() + 2 * B * lat * lat * 8 * 2) / 1e6:.2f} MB per launch', flush=True)
    res = 512
    unet, vae, sched, te, tok = load_sd15('random:sd15', None, dev, BF16)
    unet.eval().requires_grad_(False)
    prompts = [f'a photo of object number {i} on a table, studio light' for i in range(B)]
    kw = dict(guidance_scale=kappa, num_inference_steps=20, solver='dpmpp2m', init_latents=z0, start_index=0)
    runs = (('teacher_sample_solver_i2i, dpmpp2m, no mask', lambda: teacher_sample_solver_i2i(unet, z, prompts, sched, te, tok, res, **kw)),
            ('teacher_sample_solver_i2i, dpmpp2m, half mask', lambda: teacher_sample_solver_i2i(unet, z, prompts, sched, te, tok, res, mask=mask, **kw)))
    times = {name: [] for name, _ in runs}
    for rep in range(4):                    # the two runs alternate; the first round is the warm-up
        for name, fn in runs:
            torch.cuda.synchronize()
            t0 = time.time()
            fn()
            torch.cuda.synchronize()
            if rep:
                times[name].append(time.time() - t0)
    for name, v in times.items():
        med = statistics.median(v)
        print(f'(f) {name}, random:sd15, {res} x {res}, batch {B}, 20 steps, kappa {kappa}, without VAE decode: {B / med:.2f} images/s '
              f'({med:.3f} s per batch, median of 3 alternating calls after one warm-up call each; {min(v):.3f} .. {max(v):.3f} s)', flush=True)


if args.solver:
    solver_sections()
    sys.exit(0)
if args.masked:
    masked_sections()
    sys.exit(0)

moved = eps.numel() * 4 + 2 * xt.numel() * 4 + 2 * B * lat * lat * 8 * 2
variants = (('ddim_step (1 launch)', fused), ('cfg_x0 x0 + cfg_x0 raw + noisy_input (3 launches)', chain))
with torch.no_grad():
    for _, fn in variants:
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    samples = {name: [] for name, _ in variants}
    for _ in range(5):                      # the two variants alternate inside one process
        for name, fn in variants:
            samples[name].append(window_us(fn))
for name, v in samples.items():
    print(f'(a) {name}: {statistics.median(v):.1f} us per step boundary (median of 5 windows of 200 back-to-back calls, alternating with the '
          f'other variant; range {min(v):.1f} .. {max(v):.1f}); B = {B}, {lat} x {lat} latents, dup 2, bf16', flush=True)
print(f'    the fused kernel reads and writes {moved / 1e6:.2f} MB per launch', flush=True)

# ---- (b) the sampler ----
res, steps = 512, 50
unet, vae, sched, te, tok = load_sd15('random:sd15', None, dev, BF16)
unet.eval().requires_grad_(False)
prompts = [f'a photo of object number {i} on a table, studio light' for i in range(B)]
z = torch.randn(B, 4, res // 8, res // 8, generator=g).to(dev)
for decode in (False, True):
    times = []
    for rep in range(4):
        torch.cuda.synchronize()
        t0 = time.time()
        teacher_sample(unet, z, prompts, sched, te, tok, res, guidance_scale=kappa, num_inference_steps=steps, return_images=decode, vae=vae)
        torch.cuda.synchronize()
        if rep:
            times.append(time.time() - t0)
    med = statistics.median(times)
    print(f'(b) teacher_sample, random:sd15, {res} x {res}, batch {B}, {steps} steps, kappa {kappa}, {"with" if decode else "without"} VAE decode: '
          f'{B / med:.2f} images/s ({med:.2f} s per batch, median of 3 after one warm-up call; {min(times):.2f} .. {max(times):.2f} s)', flush=True)
