"""Sampling the teacher itself on the GPU: the fused DDIM step-boundary kernel (sidlsg_ddim_step) against the chain of existing
kernels it replaces, sd_util.teacher_sample against a loop composed from the public denoising entry point, the sampler's properties,
and the two command lines with the `teacher` sentinel."""
import glob
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SD = dict(steps_offset=1, set_alpha_to_one=False, timestep_spacing='leading')
EPS32 = float(torch.finfo(torch.float32).eps)

# fp32 compute mode, N = 3, kappa = 2.5, batch 2 on the seeded tiny network: relative l2 difference between teacher_sample and the
# composed loop as measured on an MI355X (test_teacher_sample_matches_the_composed_loop prints it); the test asserts 4x these.
MEASURED_FP32 = {'epsilon': 5.61e-7, 'v_prediction': 8.63e-7}


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from sid_lsg_amd._lib import lib
    lib.load()
    return torch.device('cuda:0')


def _sched(pt, dev):
    from sid_lsg_amd.scheduler import DDPMScheduler
    return DDPMScheduler(prediction_type=pt).to(dev)


def _inputs(dev, B, H, W, dup, pt='epsilon', seed=0):
    """Network output [dup*B, HW, 8] (the padding channels hold values too: the kernels must not read them into the result), x_t, and
    per-sample coefficients of three different (t, t_prev) pairs."""
    g = torch.Generator().manual_seed(seed)
    eps = torch.randn(dup * B, H * W, 8, generator=g)
    xt = torch.randn(B, 4, H, W, generator=g)
    t = torch.tensor([981, 521, 141][:B])
    sched = _sched(pt, dev)
    s0, s1 = sched.coefficients(t.to(dev))
    s0p, s1p = sched.coefficients((t - 20).to(dev))
    return eps.to(dev), xt.to(dev), s0, s1, s0p, s1p


def _nhwc(x, act):
    return x.permute(0, 2, 3, 1).to(act)


# ---- kernel ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('act', [BF16, F32])
@pytest.mark.parametrize('shape', [(8, 8), (9, 7)])
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('kappa', [1.0, 3.5])
@pytest.mark.parametrize('dup', [1, 2])
def test_ddim_step_epsilon_is_bit_equal_to_the_chain_of_existing_kernels(dev, dup, kappa, B, shape, act):
    """Mode 1: x0, x_prev and the next network input are the bits of cfg_x0(mode 1), cfg_x0(mode 0) and
    noisy_input(x0, e, s0p, s1p, dup) launched in turn; the padding channels of the next input are zero."""
    from sid_lsg_amd import ops
    eps, xt, s0, s1, s0p, s1p = _inputs(dev, B, *shape, dup)
    x0_ref = ops.cfg_x0(eps, xt, s0, s1, kappa, True, act)
    e_ref = ops.cfg_x0(eps, xt, s0, s1, kappa, False, act)
    in_ref, xtn_ref = ops.noisy_input(x0_ref, e_ref, s0p, s1p, dup, act)
    out, xtn, x0 = ops.ddim_step(eps, xt, s0, s1, s0p, s1p, kappa, act, want_x0=True)
    torch.cuda.synchronize()
    assert out.dtype == act and out.shape == in_ref.shape == (dup * B, *shape, 8)
    assert torch.equal(x0, x0_ref), float((x0 - x0_ref).abs().max())
    assert torch.equal(xtn, xtn_ref), float((xtn - xtn_ref).abs().max())
    assert torch.equal(out, in_ref)
    assert not out[..., 4:].any()
    if dup == 2:
        assert torch.equal(out[:B], out[B:])


@pytest.mark.parametrize('act', [BF16, F32])
@pytest.mark.parametrize('shape', [(8, 8), (9, 7)])
@pytest.mark.parametrize('dup,kappa', [(1, 1.0), (2, 3.5)])
def test_ddim_step_v_mode(dev, dup, kappa, shape, act):
    """Mode 2: x0 has the bits of cfg_x0(mode 2).  x_prev against an fp64 restatement that starts from the fp32 values the kernel
    works on (the guided output e, bit-equal to cfg_x0(mode 0) as the mode-1 test shows, and the kernel's own fp32 x0):
        x_prev = s0p*x0 + s1p*(s0*e + s1*x_t)
    The kernel rounds s1*x_t (product), s0*e + (.) (fma), s1p*(.) (product) and s0p*x0 + (.) (fma): with u = eps_fp32 / 2 per
    rounding the term s1p*s1*x_t passes four roundings, s1p*s0*e three and s0p*x0 one, so
        |error| <= 4 u (1 + O(u)) (|s0p x0| + |s1p s0 e| + |s1p s1 x_t|);
    the bound asserted is 4 eps_fp32 of that sum, twice the derived one.  `out` is x_prev rounded to the activation dtype."""
    from sid_lsg_amd import ops
    B = 3
    eps, xt, s0, s1, s0p, s1p = _inputs(dev, B, *shape, dup, pt='v_prediction', seed=1)
    x0_ref = ops.cfg_x0(eps, xt, s0, s1, kappa, True, act, prediction_type='v_prediction')
    e = ops.cfg_x0(eps, xt, s0, s1, kappa, False, act)
    out, xtn, x0 = ops.ddim_step(eps, xt, s0, s1, s0p, s1p, kappa, act, prediction_type='v_prediction', want_x0=True)
    torch.cuda.synchronize()
    assert torch.equal(x0, x0_ref)
    v = lambda a: a.double().view(-1, 1, 1, 1)  # noqa: E731
    a = v(s0p) * x0.double()
    b = v(s1p) * v(s0) * e.double()
    c = v(s1p) * v(s1) * xt.double()
    want = a + b + c
    bound = 4 * EPS32 * (a.abs() + b.abs() + c.abs())
    err = (xtn.double() - want).abs()
    print(f'v mode {shape} dup {dup} {act}: max error / bound = {float((err / bound).max()):.3f}')
    assert bool((err <= bound).all()), float((err / bound).max())
    assert out.dtype == act and not out[..., 4:].any()
    for d in range(dup):
        assert torch.equal(out[d * B:(d + 1) * B, ..., :4], _nhwc(xtn, act))


@pytest.mark.parametrize('act', [BF16, F32])
@pytest.mark.parametrize('pt', ['epsilon', 'v_prediction'])
@pytest.mark.parametrize('layout', ['Ce4', 'Ce5', 'offset'])
def test_ddim_step_element_load_path(dev, layout, pt, act):
    """The kernel loads the network output with two 16-byte loads when it has 8 channels and is 16-byte aligned, else element by
    element.  A 4- or 5-channel output, and an 8-channel one that starts 4 bytes into its allocation, take the second path: all
    three outputs have the bits of the vector path on the same values (and so of the chain of existing kernels)."""
    from sid_lsg_amd import ops
    B, shape, kappa = 3, (9, 7), 3.5
    eps, xt, s0, s1, s0p, s1p = _inputs(dev, B, *shape, 2, pt=pt, seed=4)
    want = ops.ddim_step(eps, xt, s0, s1, s0p, s1p, kappa, act, prediction_type=pt, want_x0=True)
    if layout == 'offset':
        buf = torch.zeros(eps.numel() + 1, device=dev)
        other = buf[1:].view(eps.shape)
        other.copy_(eps)
        assert other.is_contiguous() and other.data_ptr() % 16 == 4
    else:
        other = eps[..., :int(layout[2:])].contiguous()
    got = ops.ddim_step(other, xt, s0, s1, s0p, s1p, kappa, act, prediction_type=pt, want_x0=True)
    x0_ref = ops.cfg_x0(other, xt, s0, s1, kappa, True, act, prediction_type=pt)
    torch.cuda.synchronize()
    for g, w in zip(got, want):
        assert torch.equal(g, w)
    assert torch.equal(got[2], x0_ref)


def test_ddim_step_optional_outputs(dev):
    """The last step passes out = NULL: x_prev is the same bits and the x0 prediction too; x0 = NULL changes nothing else."""
    from sid_lsg_amd import ops
    for pt in ('epsilon', 'v_prediction'):
        eps, xt, s0, s1, s0p, s1p = _inputs(dev, 3, 9, 7, 2, pt=pt, seed=2)
        out, xtn, x0 = ops.ddim_step(eps, xt, s0, s1, s0p, s1p, 2.5, BF16, prediction_type=pt, want_x0=True)
        none, xtn_last, x0_last = ops.ddim_step(eps, xt, s0, s1, s0p, s1p, 2.5, BF16, prediction_type=pt, last=True, want_x0=True)
        out2, xtn2, none2 = ops.ddim_step(eps, xt, s0, s1, s0p, s1p, 2.5, BF16, prediction_type=pt)
        none3, xtn3, none4 = ops.ddim_step(eps, xt, s0, s1, s0p, s1p, 2.5, BF16, prediction_type=pt, last=True)
        torch.cuda.synchronize()
        assert none is None and none2 is None and none3 is None and none4 is None
        assert torch.equal(xtn_last, xtn) and torch.equal(x0_last, x0)
        assert torch.equal(out2, out) and torch.equal(xtn2, xtn) and torch.equal(xtn3, xtn)


def test_ddim_step_rejects_bad_arguments_without_a_launch(dev):
    """mode 0 / 3, dup 3 and a null eps return SIDLSG_EINVAL and launch nothing: outputs pre-filled with a sentinel stay intact."""
    from sid_lsg_amd._lib import lib
    B, HW = 2, 64
    eps, xt, s0, s1, s0p, s1p = _inputs(dev, B, 8, 8, 2)
    eps3 = torch.cat([eps, eps[:B]])
    p = lambda a: None if a is None else a.data_ptr()  # noqa: E731
    for fn, act in ((lib.sidlsg_ddim_step, BF16), (lib.sidlsg_ddim_step_f32, F32)):
        out = torch.full((2 * B, 8, 8, 8), 7.0, device=dev, dtype=act)
        out3 = torch.full((3 * B, 8, 8, 8), 7.0, device=dev, dtype=act)
        xtn, x0 = torch.full_like(xt, 7.0), torch.full_like(xt, 7.0)
        for e, o, dup, mode in ((eps, out, 2, 0), (eps, out, 2, 3), (eps3, out3, 3, 1), (None, out, 2, 1), (eps, out, 0, 1)):
            rc = fn.raw(p(e), p(xt), p(s0), p(s1), p(s0p), p(s1p), p(o), p(xtn), p(x0), B, 4, HW, 8, 8, dup, 2.0, mode, None)
            assert rc == -22, (dup, mode, rc)
        # a null x_t, coefficient or x_prev buffer, channel counts the layout cannot hold
        assert fn.raw(p(eps), None, p(s0), p(s1), p(s0p), p(s1p), p(out), p(xtn), p(x0), B, 4, HW, 8, 8, 2, 2.0, 1, None) == -22
        assert fn.raw(p(eps), p(xt), p(s0), p(s1), None, p(s1p), p(out), p(xtn), p(x0), B, 4, HW, 8, 8, 2, 2.0, 1, None) == -22
        assert fn.raw(p(eps), p(xt), p(s0), p(s1), p(s0p), p(s1p), p(out), None, p(x0), B, 4, HW, 8, 8, 2, 2.0, 1, None) == -22
        assert fn.raw(p(eps), p(xt), p(s0), p(s1), p(s0p), p(s1p), p(out), p(xtn), p(x0), B, 9, HW, 16, 16, 2, 2.0, 1, None) == -22
        assert fn.raw(p(eps), p(xt), p(s0), p(s1), p(s0p), p(s1p), p(out), p(xtn), p(x0), B, 4, HW, 2, 8, 2, 2.0, 1, None) == -22
        assert fn.raw(p(eps), p(xt), p(s0), p(s1), p(s0p), p(s1p), p(out), p(xtn), p(x0), B, 4, HW, 8, 12, 2, 2.0, 1, None) == -22
        torch.cuda.synchronize()
        for buf in (out, out3, xtn, x0):
            assert bool((buf == 7.0).all())


def test_ddim_step_keeps_a_nan_inside_its_sample(dev):
    """A NaN in one sample's network output: that sample's outputs are NaN, the other samples' outputs keep their bits."""
    from sid_lsg_amd import ops
    for pt in ('epsilon', 'v_prediction'):
        eps, xt, s0, s1, s0p, s1p = _inputs(dev, 3, 8, 8, 2, pt=pt, seed=3)
        clean = ops.ddim_step(eps, xt, s0, s1, s0p, s1p, 3.5, BF16, prediction_type=pt, want_x0=True)
        bad = eps.clone()
        bad[1, 5, 2] = float('nan')            # sample 1, unconditional half
        got = ops.ddim_step(bad, xt, s0, s1, s0p, s1p, 3.5, BF16, prediction_type=pt, want_x0=True)
        torch.cuda.synchronize()
        out, xtn, x0 = got
        assert torch.isnan(xtn[1]).any() and torch.isnan(x0[1]).any() and torch.isnan(out[1].float()).any() and torch.isnan(out[4].float()).any()
        keep = [0, 2]
        assert torch.equal(xtn[keep], clean[1][keep]) and torch.equal(x0[keep], clean[2][keep])
        assert torch.equal(out[[0, 2, 3, 5]], clean[0][[0, 2, 3, 5]])


def test_ddim_step_is_forward_only(dev):
    from sid_lsg_amd import ops
    eps, xt, s0, s1, s0p, s1p = _inputs(dev, 1, 8, 8, 1)
    with pytest.raises(RuntimeError, match='forward only'):
        ops.ddim_step(eps.requires_grad_(True), xt, s0, s1, s0p, s1p, 1.0)
    with torch.no_grad():
        ops.ddim_step(eps, xt, s0, s1, s0p, s1p, 1.0)
    with pytest.raises(RuntimeError, match='does not match'):
        ops.ddim_step(eps.detach()[:, :10], xt, s0, s1, s0p, s1p, 1.0)


# ---- sampler --------------------------------------------------------------------------------------------------------------------
PROMPTS = ['a red cube on a table', 'two blue spheres']
_models = {}


def _model(dev, pt, cd):
    """The seeded tiny network (random:tiny / random:tiny:v) with its text encoder, tokenizer, VAE and scheduler; built once."""
    key = (pt, cd)
    if key not in _models:
        from sid_lsg_amd.sd_util import load_sd15
        spec = 'random:tiny' if pt == 'epsilon' else 'random:tiny:v'
        unet, vae, sched, te, tok = load_sd15(spec, None, dev, F32, compute_dtype=cd)
        unet.eval().requires_grad_(False)
        _models[key] = (unet, vae, sched, te, tok)
    return _models[key]


def _z(dev, b=2, lat=8, seed=11):
    return torch.randn(b, 4, lat, lat, generator=torch.Generator().manual_seed(seed)).to(dev)


def _composed(dev, pt, cd, z, N, kappa):
    """The same sampler from public existing pieces: per step sid_sd_denoise(predict_x0=True) and sid_sd_denoise(predict_x0=False) at
    t_i on x_{t_i} = add_noise(x0_{i-1}, eps_hat_{i-1}, t_i) -- which is DDIM's own x_prev, given to sid_sd_denoise as its (images,
    noise) pair -- then eps_hat and x_prev = add_noise(x0, eps_hat, t_prev) in fp64 torch arithmetic.  x_T = z is given as the pair
    (s0 z, s1 z): s0^2 + s1^2 = 1 to fp32 rounding.
    The timesteps and coefficients are ddim_schedule's own, so this comparison checks the loop and the kernel, not the schedule: that
    is pinned against the published formulas in tests/test_teacher_sampler_host.py."""
    from sid_lsg_amd.scheduler import ddim_schedule
    from sid_lsg_amd.sd_util import sid_sd_denoise
    unet, _, sched, te, tok = _model(dev, pt, cd)
    ts, s0, s1, s0p, s1p = (v.double() if v.is_floating_point() else v for v in ddim_schedule(sched, SD, N))
    assert torch.equal(s0p[:-1], s0[1:]) and torch.equal(s1p[:-1], s1[1:])       # t_prev of step i is t_{i+1}
    img, noi = (s0[0] * z.double()).float(), (s1[0] * z.double()).float()
    for i in range(N):
        t = ts[i].expand(len(z)).contiguous()
        kw = dict(unet=unet, images=img, noise=noi, contexts=PROMPTS, timesteps=t, noise_scheduler=sched, text_encoder=te, tokenizer=tok,
                  resolution=64, dtype=F32, guidance_scale=kappa)
        x0 = sid_sd_denoise(predict_x0=True, **kw).double()
        e = sid_sd_denoise(predict_x0=False, **kw).double()
        if pt == 'v_prediction':
            e = s0[i] * e + s1[i] * (s0[i] * img.double() + s1[i] * noi.double())
        x_prev = s0p[i] * x0 + s1p[i] * e
        img, noi = x0.float(), e.float()
    return x_prev


def _rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@pytest.mark.parametrize('pt', ['epsilon', 'v_prediction'])
def test_teacher_sample_matches_the_composed_loop(dev, pt):
    """fp32 compute mode, N = 3, kappa = 2.5, batch 2: relative l2 difference of the final latent against the composed loop.  Measured
    on an MI355X: 5.61e-7 (epsilon), 8.63e-7 (v) -- MEASURED_FP32; asserted at most 4x that, which must itself stay below 1e-5 * N (the
    fp32 mode is specified at 1e-6 per call against the oracle, so anything near that cap is a defect, not noise).
    The same comparison in bf16 mode measured 8.0e-8 (epsilon) and 9.3e-8 (v): both sides run the same bf16 network and the glue's
    fp32 roundings rarely move an input across a bf16 step.  It is printed, and asserted below the fp32 bound x 2^8.5, which the
    measured values support with a wide margin.  (bf16 against fp32 mode: 5.3e-3 / 7.9e-3, printed only.)"""
    from sid_lsg_amd.sd_util import teacher_sample
    N, kappa = 3, 2.5
    z = _z(dev)
    unet, _, sched, te, tok = _model(dev, pt, F32)
    got = teacher_sample(unet, z, PROMPTS, sched, te, tok, 64, guidance_scale=kappa, num_inference_steps=N)
    want = _composed(dev, pt, F32, z, N, kappa)
    torch.cuda.synchronize()
    assert got.dtype == F32 and got.shape == z.shape and bool(torch.isfinite(got).all())
    rel = _rel_l2(got, want)
    bound = 4 * MEASURED_FP32[pt]
    print(f'teacher_sample vs composed loop, fp32 mode, {pt}: relative l2 {rel:.3e} (bound {bound:.1e})')
    assert bound <= 1e-5 * N
    assert rel <= bound, rel
    # the sampler moved the latent: three guided steps are not the identity
    assert _rel_l2(got, z) > 1e-2
    unet_b, _, sched_b, te_b, tok_b = _model(dev, pt, BF16)
    got_b = teacher_sample(unet_b, z, PROMPTS, sched_b, te_b, tok_b, 64, guidance_scale=kappa, num_inference_steps=N)
    want_b = _composed(dev, pt, BF16, z, N, kappa)
    torch.cuda.synchronize()
    rel_b = _rel_l2(got_b, want_b)
    print(f'teacher_sample vs composed loop, bf16 mode, {pt}: relative l2 {rel_b:.3e}; against the fp32 mode {_rel_l2(got_b, got):.3e}')
    assert bool(torch.isfinite(got_b).all()) and np.isfinite(rel_b)
    assert rel_b <= bound * 2 ** 8.5, rel_b


def test_teacher_sample_without_guidance_makes_no_unconditional_pass(dev, monkeypatch):
    """kappa = 1: the same bits whatever the unconditional prompt would encode to, because it is never encoded (dup = 1); with
    kappa = 2 the substituted prompt does change the result, so the substitution bites."""
    from sid_lsg_amd import sd_util
    unet, _, sched, te, tok = _model(dev, 'epsilon', BF16)
    z = _z(dev)
    run = lambda k: sd_util.teacher_sample(unet, z, PROMPTS, sched, te, tok, 64, guidance_scale=k, num_inference_steps=2)  # noqa: E731
    plain1, plain2 = run(1), run(2.0)
    orig, seen = sd_util.encode_contexts, []

    def other_uncond(contexts, *a, **kw):
        if not torch.is_tensor(contexts) and all(c == '' for c in contexts):
            seen.append(len(contexts))
            contexts = ['something else entirely'] * len(contexts)
        return orig(contexts, *a, **kw)
    monkeypatch.setattr(sd_util, 'encode_contexts', other_uncond)
    sub1 = run(1)
    assert seen == []
    sub2 = run(2.0)
    torch.cuda.synchronize()
    assert seen == [2]
    assert torch.equal(sub1, plain1)
    assert not torch.equal(sub2, plain2)
    assert not torch.equal(plain1, plain2)


@pytest.mark.parametrize('pt', ['epsilon', 'v_prediction'])
def test_one_step_to_alpha_one_returns_the_x0_prediction(dev, pt):
    """N = 1 with set_alpha_to_one: x_prev = 1 * x0 + 0 * eps_hat, exactly the cfg_x0 x0 prediction of a single guided pass at t_0."""
    from sid_lsg_amd import ops
    from sid_lsg_amd.sd_util import encode_contexts, teacher_sample
    unet, _, sched, te, tok = _model(dev, pt, BF16)
    z = _z(dev)
    cfg = dict(SD, set_alpha_to_one=True)
    got = teacher_sample(unet, z, PROMPTS, sched, te, tok, 64, guidance_scale=2.5, num_inference_steps=1, schedule_config=cfg)
    t = torch.full((2,), 1, dtype=torch.long, device=dev)
    s0, s1 = sched.coefficients(t)
    ones = torch.ones(2, device=dev)
    ctx = torch.cat([encode_contexts([''] * 2, te, tok, dev), encode_contexts(PROMPTS, te, tok, dev)]).to(BF16).contiguous()
    xin, xt = ops.noisy_input(None, z, ones, ones, 2, BF16)
    eps = unet.forward_nhwc(xin, torch.cat([t, t]), ctx)
    want = ops.cfg_x0(eps, xt, s0, s1, 2.5, True, BF16, prediction_type=pt)
    torch.cuda.synchronize()
    assert torch.equal(xt, z)
    assert torch.equal(got, want)


def test_teacher_sample_loop_issues_device_work_only(dev, monkeypatch):
    """From the first UNet pass to the return of the latent, nothing waits for the device: torch.cuda.synchronize, stream / event
    synchronize, Tensor.item / .cpu / .tolist / .numpy are patched to count, and torch's own synchronisation detector
    (torch.cuda.set_sync_debug_mode('error')) is on for the span, so a blocking copy or a data-dependent host decision raises."""
    from sid_lsg_amd import sd_util
    unet, _, sched, te, tok = _model(dev, 'epsilon', BF16)
    z = _z(dev)
    N = 4
    want = sd_util.teacher_sample(unet, z, PROMPTS, sched, te, tok, 64, guidance_scale=2.5, num_inference_steps=N)     # warm: allocations, lazy loads
    torch.cuda.synchronize()
    state = dict(inside=False, passes=0, syncs=[])

    def counting(name, fn):
        def wrapper(*a, **kw):
            if state['inside']:
                state['syncs'].append(name)
            return fn(*a, **kw)
        return wrapper
    monkeypatch.setattr(torch.cuda, 'synchronize', counting('torch.cuda.synchronize', torch.cuda.synchronize))
    monkeypatch.setattr(torch.cuda.Stream, 'synchronize', counting('Stream.synchronize', torch.cuda.Stream.synchronize))
    monkeypatch.setattr(torch.cuda.Event, 'synchronize', counting('Event.synchronize', torch.cuda.Event.synchronize))
    for name in ('item', 'cpu', 'tolist', 'numpy'):
        monkeypatch.setattr(torch.Tensor, name, counting(f'Tensor.{name}', getattr(torch.Tensor, name)))
    forward = unet.forward_nhwc

    def first_pass_opens_the_span(*a, **kw):
        if not state['inside']:
            state['inside'] = True
            torch.cuda.set_sync_debug_mode('error')
        state['passes'] += 1
        return forward(*a, **kw)
    monkeypatch.setattr(unet, 'forward_nhwc', first_pass_opens_the_span)
    try:
        got = sd_util.teacher_sample(unet, z, PROMPTS, sched, te, tok, 64, guidance_scale=2.5, num_inference_steps=N)
    finally:
        torch.cuda.set_sync_debug_mode('default')
        state['inside'] = False
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert state['passes'] == N and state['syncs'] == []
    assert torch.equal(got, want)


def test_teacher_sample_decodes_as_the_one_step_sampler_does(dev):
    """return_images: vae.decode(latent / scaling_factor), float32, the image size of the resolution."""
    from sid_lsg_amd.sd_util import teacher_sample
    unet, vae, sched, te, tok = _model(dev, 'epsilon', BF16)
    z = _z(dev)
    lat = teacher_sample(unet, z, PROMPTS, sched, te, tok, 64, guidance_scale=2.0, num_inference_steps=2)
    img = teacher_sample(unet, z, PROMPTS, sched, te, tok, 64, guidance_scale=2.0, num_inference_steps=2, return_images=True, vae=vae)
    want = vae.decode(lat.to(vae.dtype) / vae.config.scaling_factor, return_dict=False)[0].to(F32)
    torch.cuda.synchronize()
    assert img.dtype == F32 and img.shape == (2, 3, 64, 64)
    assert torch.equal(img, want)


# ---- command lines --------------------------------------------------------------------------------------------------------------
def _png_pixels(path):
    import PIL.Image
    return np.asarray(PIL.Image.open(path).convert('RGB'))


def test_generate_onestep_samples_the_teacher(dev, tmp_path):
    """`generate_onestep.py --network teacher` in a child process: two PNG files of the requested size, named by their seeds; another
    step count gives other pixels (second run in this process, as tests/test_gpu_cli.py runs the command)."""
    from click.testing import CliRunner
    import generate_onestep
    prompts = tmp_path / 'prompts.txt'
    prompts.write_text('a red cube\na blue sphere\n')
    common = ['--network', 'teacher', '--repo_id', 'random:tiny', '--guidance_scale', '2', '--seeds', '0-1', '--resolution', '64',
              '--text_prompts', str(prompts), '--num_steps_eval', '2']
    out3, out2 = tmp_path / 'steps3', tmp_path / 'steps2'
    with socket.socket() as sock:           # a rendezvous port of the child's own: this process may hold the default one
        sock.bind(('127.0.0.1', 0))
        port = sock.getsockname()[1]
    res = subprocess.run([sys.executable, os.path.join(ROOT, 'generate_onestep.py'), '--outdir', str(out3), '--teacher_steps', '3'] + common,
                         cwd=ROOT, capture_output=True, text=True, timeout=240, env=dict(os.environ, MASTER_PORT=str(port)))
    assert res.returncode == 0, res.stdout + res.stderr
    assert 'DDIM 3 steps, guidance scale 2' in res.stdout and '--num_steps_eval 2 is ignored' in res.stdout
    files = sorted(glob.glob(str(out3 / '*.png')))
    assert [os.path.basename(f) for f in files] == ['000000.png', '000001.png'] and not glob.glob(str(tmp_path / '*numstep*'))
    a = [_png_pixels(f) for f in files]
    for img in a:
        assert img.shape == (64, 64, 3) and img.dtype == np.uint8 and img.min() != img.max()
    assert not np.array_equal(a[0], a[1])
    r2 = CliRunner().invoke(generate_onestep.main, ['--outdir', str(out2), '--teacher_steps', '2'] + common, catch_exceptions=False)
    assert r2.exit_code == 0, r2.output
    b = [_png_pixels(f) for f in sorted(glob.glob(str(out2 / '*.png')))]
    assert len(b) == 2 and all(x.shape == (64, 64, 3) for x in b)
    assert not np.array_equal(a[0], b[0]) and not np.array_equal(a[1], b[1])


def test_sid_train_evaluates_the_teacher_once(dev, tmp_path):
    """`sid_train.py --train_mode 0 --network_pkl teacher --metrics fid_test` with the detector and statistics stand-ins of
    tests/test_gpu_cli.py: one report line with snapshot_pkl teacher-ddim3-cfg2, no 1 / 2 / 4 loop, one preview grid."""
    from click.testing import CliRunner
    import sid_train
    from sid_lsg_amd.preview import grid_layout

    class Detector(torch.nn.Module):
        def __init__(self):
            super().__init__()
            torch.manual_seed(0)
            self.conv = torch.nn.Conv2d(3, 16, 8, stride=8)

        def forward(self, img: torch.Tensor, return_features: bool = True) -> torch.Tensor:
            return self.conv(img.to(torch.float32) / 255.0).mean(dim=(2, 3))
    det_path, stat_path = str(tmp_path / 'detector.pt'), str(tmp_path / 'real_stats.npz')
    torch.jit.script(Detector()).save(det_path)
    np.savez(stat_path, mu=np.zeros(16), sigma=np.eye(16) * 0.01)
    (tmp_path / 'aesthetics_6_plus.txt').write_text('\n'.join(f'prompt number {i}' for i in range(40)) + '\n')
    caps = tmp_path / 'coco_captions.txt'
    caps.write_text('\n'.join(f'evaluation caption {i}' for i in range(9)) + '\n')
    runs = tmp_path / 'runs'
    ev = CliRunner().invoke(sid_train.main, [
        '--outdir', str(runs), '--data_prompt_text', str(tmp_path), '--data', str(caps), '--sd_model', 'random:tiny', '--seed', '1',
        '--resolution', '64', '--batch', '8', '--batch-gpu', '8', '--train_mode', '0', '--network_pkl', 'teacher', '--teacher_steps', '3',
        '--teacher_cfg', '2', '--metrics', 'fid_test', '--metric_pt_path', det_path, '--data_stat', stat_path, '--snapshot_images', '1'],
        catch_exceptions=False)
    assert ev.exit_code == 0, ev.output
    run_dir = glob.glob(str(runs / '00000-*'))[0]
    files = glob.glob(os.path.join(run_dir, 'metric-fid_test*.jsonl'))
    assert [os.path.basename(f) for f in files] == ['metric-fid_test.jsonl']
    rows = [json.loads(ln) for ln in open(files[0])]
    assert len(rows) == 1 and rows[0]['snapshot_pkl'] == 'teacher-ddim3-cfg2' and rows[0]['metric'] == 'fid_test'
    assert np.isfinite(rows[0]['results']['fid30k_full']) and rows[0]['results']['fid30k_full'] > 0
    # once: no per-step-count result files of the snapshot branch, one grid
    assert not glob.glob(str(runs / 'fid_test*_[124].txt')) and not glob.glob(os.path.join(run_dir, 'fid_test*_[124].png'))
    grid = os.path.join(run_dir, 'fid_test_teacher.png')
    assert os.path.isfile(grid)
    px = _png_pixels(grid)
    (gw, gh), _ = grid_layout(9, 64)                # 32 x 32 tiles at this resolution
    assert px.shape == (gh * 64, gw * 64, 3) and px.min() != px.max()
