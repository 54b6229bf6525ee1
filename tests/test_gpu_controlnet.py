"""ControlNet conditioning on the GPU (sid_lsg_amd.controlnet, HipUNet2DCondition.forward_nhwc(control=...), the samplers, the command
line) against the fp64 torch.nn restatement of tests/controlnet_ref.py.  The HIP modules and the reference load one state dict through
their diffusers key names.  tests/test_controlnet_host.py asserts the precondition: the seeded ControlNet used here changes the
reference's output by more than 10 %, so no tolerance below can be met by ignoring the control state.

Shapes: B = 3 with distinct timesteps.  The ControlNet's own features are checked at NON-square 8 x 12 latents (control images 64 x 96; the
stride-2 stages see 12 -> 6 -> 3 -> 2).  A UNet pass cannot run there: its up path doubles 2 back to 4, not 3, so a four-level UNet needs
sides that are multiples of 8; the UNet tests use 8 x 16 latents (control images 64 x 128), still non-square."""
import glob
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import controlnet_ref as cr

pytestmark = pytest.mark.gpu
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP32_TOL = 1e-4      # max |err| / max |ref|: the bound of tests/test_gpu_fp32.py::test_unet_forward_backward_f32 for a UNet forward of these configs


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from sid_lsg_amd._lib import lib
    lib.load()
    return torch.device('cuda:0')


def close(got, ref, tol, name=''):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, f'{name}: shape {tuple(got.shape)} vs {tuple(ref.shape)}'
    assert torch.isfinite(got).all(), f'{name}: non-finite output'
    err, scale = (got - ref).abs().max().item(), ref.abs().max().item() + 1e-30
    assert err <= tol * scale, f'{name}: max err {err:.4g} vs scale {scale:.4g} (rel {err / scale:.3g} > {tol})'
    return err / scale


def rel_l2(got, ref):
    return float((got.detach().double().cpu() - ref.double()).norm() / ref.double().norm())


_refs, _nets = {}, {}


def ref_pair(name):
    """(ControlledUNetRef, ControlNetRef, unet state dict, controlnet state dict) in fp64, built once per configuration."""
    if name not in _refs:
        _refs[name] = cr.make_pair(name)
    return _refs[name]


def hip_pair(name, cd, dev):
    """(HipUNet2DCondition, HipControlNet) of compute dtype `cd` holding the reference's weights, built once."""
    from sid_lsg_amd.controlnet import HipControlNet
    from sid_lsg_amd.unet import CONFIGS, HipUNet2DCondition
    if (name, cd) not in _nets:
        _, _, usd, csd = ref_pair(name)
        unet = HipUNet2DCondition(CONFIGS[name], compute_dtype=cd).materialize(dev, with_grad_buffers=False, source=usd).requires_grad_(False)
        _nets[(name, cd)] = (unet, HipControlNet(CONFIGS[name], compute_dtype=cd).materialize(dev, source=csd))
    return _nets[(name, cd)]


def nhwc8(x, cd, dev):
    """[B, 4, h, w] -> the UNet's input [B, h, w, 8] of the compute dtype, channels 4..7 zero."""
    B, C, h, w = x.shape
    out = torch.zeros(B, h, w, 8)
    out[..., :C] = x.permute(0, 2, 3, 1)
    return out.to(cd).to(dev)


def nchw(eps, h, w):
    """forward_nhwc's [B, h*w, 8] -> [B, 4, h, w] on the CPU."""
    return eps.view(eps.shape[0], h, w, 8)[..., :4].permute(0, 3, 1, 2).cpu()


def run_unet(unet, x, t, ctx, dev, control=None):
    """One pass on CPU inputs -> [B, 4, h, w] on the CPU; without a control state the call has no `control` argument at all."""
    h, w = x.shape[2:]
    args = (nhwc8(x, unet.compute_dtype, dev), t.to(dev), ctx.to(unet.compute_dtype).to(dev).contiguous())
    with torch.no_grad():
        eps = unet.forward_nhwc(*args) if control is None else unet.forward_nhwc(*args, control=control)
    return nchw(eps, h, w)


# ---- 1. the conversion kernel ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [BF16, F32])
@pytest.mark.parametrize('shape', [(2, 64, 96), (3, 24, 40)])
def test_control_hint_u8_is_bit_exact(dev, shape, dtype):
    """Every byte value, against (img.float() / 255).to(dtype) formed on the host (one IEEE fp32 division; bf16: rounded to nearest even).
    Channels 3..7 are exactly zero."""
    from sid_lsg_amd import ops
    B, H, W = shape
    n = B * H * W * 3
    img = torch.arange(n, dtype=torch.int64).remainder(256).to(torch.uint8).view(B, H, W, 3)
    img[-1] = torch.randint(0, 256, (H, W, 3), generator=torch.Generator().manual_seed(0), dtype=torch.uint8)
    assert len(torch.unique(img)) == 256
    got = ops.control_hint_u8(img.to(dev), dtype).cpu()
    want = torch.zeros(B, H, W, 8, dtype=dtype)
    want[..., :3] = (img.float() / 255).to(dtype)
    bits = torch.int16 if dtype == BF16 else torch.int32
    assert got.dtype == dtype and got.shape == want.shape
    assert torch.equal(got.view(bits), want.view(bits))
    assert not got[..., 3:].view(bits).any()
    with pytest.raises(RuntimeError):
        ops.control_hint_u8(img.permute(0, 3, 1, 2).contiguous().to(dev), dtype)


# ---- 2. hint embedder and the thirteen features, fp32 mode --------------------------------------------------------------------------
@pytest.mark.parametrize('name,dup', [('tiny', 1), ('tiny21', 1), ('tiny', 2)])
def test_features_match_the_reference_f32(dev, name, dup):
    """8 x 12 latents, control images 64 x 96.  dup = 2: the [uncond ; cond] batch (distinct text states per half) gets the same hint twice."""
    _, cnet, _, _ = ref_pair(name)
    _, net = hip_pair(name, F32, dev)
    x, t, ctx, img = cr.make_inputs(name, w=12)
    cond = (img.double() / 255).permute(0, 3, 1, 2)
    if dup == 2:
        x, t, cond = torch.cat([x, x]), torch.cat([t, t]), torch.cat([cond, cond])
        ctx = torch.cat([torch.randn(ctx.shape, generator=torch.Generator().manual_seed(9)).to(BF16).float(), ctx])
    with torch.no_grad():
        want_e = cnet.embed(cond)
        want = cnet.features(x.double(), t, ctx.double(), cond)
        state = net.prepare(img.to(dev), 1.0, dup=dup)
        got = net.features(nhwc8(x, F32, dev), t.to(dev), ctx.to(dev), state.e)
    assert state.e.shape == (dup * 3, 8, 12, want_e.shape[1]) and state.e.dtype == F32
    worst = close(state.e.permute(0, 3, 1, 2), want_e, FP32_TOL, 'hint embedding')
    assert len(got) == len(want) == 13
    for i, (g, r) in enumerate(zip(got, want)):
        worst = max(worst, close(g.permute(0, 3, 1, 2), r, FP32_TOL, f'feature {i}'))
    assert got[-1].shape[1:3] == (1, 2) and got[6].shape[1:3] == (2, 3)       # 12 -> 6 -> 3 -> 2: the stride-2 output sizes
    print(f'{name} dup {dup}: hint embedding and 13 features, fp32 mode: worst max-norm error {worst:.2e}')


# ---- 3. UNet with control, fp32 mode ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('scale', [1.0, 0.5])
@pytest.mark.parametrize('name', ['tiny', 'tiny21'])
def test_controlled_unet_matches_the_reference_f32(dev, name, scale):
    uref, cref, _, _ = ref_pair(name)
    unet, net = hip_pair(name, F32, dev)
    x, t, ctx, img = cr.make_inputs(name, w=16)
    plain, want = cr.ref_outputs(uref, cref, x, t, ctx, img, scale)
    got = run_unet(unet, x, t, ctx, dev, control=net.prepare(img.to(dev), scale))
    e = close(got, want, FP32_TOL, 'controlled UNet')
    print(f'{name} scale {scale}: controlled UNet, fp32 mode: max-norm error {e:.2e}; control effect {rel_l2(want, plain):.3f}')
    assert rel_l2(got, plain) > 0.05


# ---- 4. bf16: at most twice the error of the plain bf16 UNet --------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['tiny', 'tiny21'])
def test_controlled_unet_bf16_error_is_at_most_twice_the_plain_error(dev, name):
    """Relative l2 error against fp64 of the controlled bf16 output <= 2 x that of the UNCHANGED plain bf16 UNet on the same inputs: a
    second bf16 network of equal depth feeds every skip connection, so independent errors of equal size would give sqrt(2).
    Both figures are printed (-s).  Measured on an MI355X (profiles/controlnet.txt): tiny plain 1.094e-2, controlled 1.001e-2 (0.92 x);
    tiny21 plain 1.112e-2, controlled 1.030e-2 (0.93 x)."""
    uref, cref, _, _ = ref_pair(name)
    unet, net = hip_pair(name, BF16, dev)
    x, t, ctx, img = cr.make_inputs(name, w=16)
    plain, want = cr.ref_outputs(uref, cref, x, t, ctx, img, 1.0)
    e_plain = rel_l2(run_unet(unet, x, t, ctx, dev), plain)
    got = run_unet(unet, x, t, ctx, dev, control=net.prepare(img.to(dev), 1.0))
    e_ctl = rel_l2(got, want)
    print(f'{name} bf16: plain UNet rel l2 {e_plain:.3e}, controlled {e_ctl:.3e}, ratio {e_ctl / e_plain:.2f}')
    assert torch.isfinite(got).all() and e_plain > 0
    assert e_ctl <= 2 * e_plain


# ---- 5. bit-exact invariances ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cd', [BF16, F32])
def test_bit_exact_invariances(dev, cd):
    from sid_lsg_amd.controlnet import HipControlNet
    from sid_lsg_amd.unet import CONFIGS
    name = 'tiny'
    _, _, _, csd = ref_pair(name)
    unet, net = hip_pair(name, cd, dev)
    x, t, ctx, img = cr.make_inputs(name, w=16)
    img = img.to(dev)
    plain = run_unet(unet, x, t, ctx, dev)
    with torch.no_grad():
        xin, tt, cc = nhwc8(x, cd, dev), t.to(dev), ctx.to(cd).to(dev)
        assert torch.equal(nchw(unet.forward_nhwc(xin, tt, cc, control=None), 8, 16), plain)           # control=None is the call without it
        assert torch.equal(nchw(unet.forward_nhwc(xin, tt, cc, None), 8, 16), plain)
    full = run_unet(unet, x, t, ctx, dev, control=net.prepare(img, 1.0))
    assert not torch.equal(full, plain)
    # scale 0 takes the plain path
    assert torch.equal(run_unet(unet, x, t, ctx, dev, control=net.prepare(img, 0.0)), plain)
    # thirteen zero taps (weights and biases): injection is res + 0 and nothing else
    tap = lambda k: k.startswith(('controlnet_down_blocks.', 'controlnet_mid_block.'))      # noqa: E731
    zero = HipControlNet(CONFIGS[name], compute_dtype=cd).materialize(dev, source={k: (torch.zeros_like(v) if tap(k) else v) for k, v in csd.items()})
    assert sum(tap(k) for k in csd) == 26
    assert torch.equal(run_unet(unet, x, t, ctx, dev, control=zero.prepare(img, 1.0)), plain)
    # scale s == scale 1 of a ControlNet whose tap weights and biases were multiplied by s in fp32 (and then cast, by its own refresh)
    s = 0.7
    pre = HipControlNet(CONFIGS[name], compute_dtype=cd).materialize(
        dev, source={k: (v * torch.tensor(s, dtype=F32) if tap(k) else v) for k, v in csd.items()})
    a = run_unet(unet, x, t, ctx, dev, control=net.prepare(img, s))
    b = run_unet(unet, x, t, ctx, dev, control=pre.prepare(img, 1.0))
    assert torch.equal(a, b) and not torch.equal(a, full) and not torch.equal(a, plain)
    # zeroing the taps of a live network in place is seen by the next prepare (the compute copies follow the masters)
    with torch.no_grad():
        for m in pre._taps():
            m.weight.zero_()
            m.bias.zero_()
    assert torch.equal(run_unet(unet, x, t, ctx, dev, control=pre.prepare(img, 1.0)), plain)


def test_refusals_on_the_gpu(dev):
    from sid_lsg_amd import ops
    from sid_lsg_amd.controlnet import HipControlNet
    from sid_lsg_amd.unet import CONFIGS, HipUNet2DCondition
    unet, net = hip_pair('tiny', BF16, dev)
    x, t, ctx, img = cr.make_inputs('tiny', w=16)
    state = net.prepare(img.to(dev), 1.0)
    xin, tt, cc = nhwc8(x, BF16, dev), t.to(dev), ctx.to(BF16).to(dev)
    with pytest.raises(RuntimeError, match='autograd'):
        unet.forward_nhwc(xin, tt, cc, control=state)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match='grouped pass'):
            with ops.dual_networks({}):
                unet.forward_nhwc(xin, tt, cc, control=state)
        with pytest.raises(ValueError, match='8h x 8w'):                       # 64 x 128 control images for 8 x 8 latents
            unet.forward_nhwc(xin[:, :, :8].contiguous(), tt, cc, control=state)
        with pytest.raises(ValueError, match='dup'):                           # a guided batch with a dup = 1 state
            unet.forward_nhwc(torch.cat([xin, xin]), torch.cat([tt, tt]), torch.cat([cc, cc]), control=state)
        other = HipUNet2DCondition(CONFIGS['tiny21'], compute_dtype=BF16).materialize(dev, with_grad_buffers=False).requires_grad_(False)
        c21 = torch.zeros(3, 77, 128, dtype=BF16, device=dev)
        with pytest.raises(ValueError, match='block_out_channels'):
            other.forward_nhwc(xin, tt, c21, control=state)
        f32net = HipControlNet(CONFIGS['tiny'], compute_dtype=F32).materialize(dev, seed=0)
        with pytest.raises(RuntimeError, match='computes in'):
            unet.forward_nhwc(xin, tt, cc, control=f32net.prepare(img.to(dev), 1.0))
        with pytest.raises(RuntimeError, match='not supported'):
            net.enable_fp8_weights()


# ---- 6. samplers ------------------------------------------------------------------------------------------------------------------------
# teacher_sample / teacher_sample_solver keep the signatures the suite pins (tests/test_teacher_sampler_host.py, tests/test_solver_host.py): as
# with init_latents / mask, the new argument lives on teacher_sample_i2i / teacher_sample_solver_i2i, which the old names call.
PROMPTS = ['a red cube on a table', 'two blue spheres']
_model = {}


def model(dev):
    """random:tiny with its text encoder, tokenizer and scheduler (bf16), a seeded ControlNet for it and two 64 x 64 control images."""
    if not _model:
        from sid_lsg_amd.sd_util import load_controlnet, load_sd15
        unet, vae, sched, te, tok = load_sd15('random:tiny', None, dev, F32, compute_dtype=BF16)
        unet.eval().requires_grad_(False)
        net = load_controlnet('random:controlnet:3', unet, dev)
        img = torch.randint(0, 256, (2, 64, 64, 3), generator=torch.Generator().manual_seed(4), dtype=torch.uint8).to(dev)
        _model.update(unet=unet, sched=sched, te=te, tok=tok, net=net, img=img)
    m = _model
    return m['unet'], m['sched'], m['te'], m['tok'], m['net'], m['img']


def _z(dev, seed=11):
    return torch.randn(2, 4, 8, 8, generator=torch.Generator().manual_seed(seed)).to(dev)


def _guided_ctx(te, tok, dev):
    from sid_lsg_amd.sd_util import encode_contexts
    return torch.cat([encode_contexts([''] * 2, te, tok, dev), encode_contexts(PROMPTS, te, tok, dev)]).to(BF16).contiguous()


def test_teacher_sample_with_control_is_the_hand_written_loop(dev):
    from sid_lsg_amd import ops
    from sid_lsg_amd.scheduler import ddim_schedule
    from sid_lsg_amd.sd_util import sampling_config_of, teacher_sample, teacher_sample_i2i
    unet, sched, te, tok, net, img = model(dev)
    z, N, kappa, b = _z(dev), 3, 2.5, 2
    state = net.prepare(img, 1.0, dup=2)
    got = teacher_sample_i2i(unet, z, PROMPTS, sched, te, tok, 64, guidance_scale=kappa, num_inference_steps=N, control=state)
    plain = teacher_sample(unet, z, PROMPTS, sched, te, tok, 64, guidance_scale=kappa, num_inference_steps=N)
    with torch.no_grad():
        ts, s0, s1, s0p, s1p = (v.to(dev) for v in ddim_schedule(sched, sampling_config_of(sched), N))
        row = lambda v, i: v.to(F32)[i].expand(b).contiguous()      # noqa: E731
        ctx, ones = _guided_ctx(te, tok, dev), torch.ones(b, device=dev)
        xin, xt = ops.noisy_input(None, z, ones, ones, 2, BF16)
        for i in range(N):
            eps = unet.forward_nhwc(xin, ts[i].expand(2 * b).contiguous(), ctx, control=state)
            xin, xt, _ = ops.ddim_step(eps, xt, row(s0, i), row(s1, i), row(s0p, i), row(s1p, i), kappa, BF16, prediction_type='epsilon', last=i == N - 1)
    torch.cuda.synchronize()
    assert torch.equal(got, xt)
    assert torch.isfinite(got).all() and not torch.equal(got, plain)
    assert torch.equal(teacher_sample_i2i(unet, z, PROMPTS, sched, te, tok, 64, guidance_scale=kappa, num_inference_steps=N,
                                          control=net.prepare(img, 0.0, dup=2)), plain)


def test_teacher_sample_solver_with_control_is_the_hand_written_loop(dev):
    from sid_lsg_amd import ops
    from sid_lsg_amd.scheduler import solver_schedule
    from sid_lsg_amd.sd_util import sampling_config_of, teacher_sample_solver, teacher_sample_solver_i2i
    unet, sched, te, tok, net, img = model(dev)
    z, N, kappa, b = _z(dev), 3, 2.5, 2
    state = net.prepare(img, 0.8, dup=2)
    kw = dict(guidance_scale=kappa, num_inference_steps=N, solver='dpmpp2m')
    got = teacher_sample_solver_i2i(unet, z, PROMPTS, sched, te, tok, 64, control=state, **kw)
    plain = teacher_sample_solver(unet, z, PROMPTS, sched, te, tok, 64, **kw)
    with torch.no_grad():
        ts, s0, s1, coef = solver_schedule(sched, sampling_config_of(sched), N, solver='dpmpp2m', spacing=None, eta=0.0, start=0)
        flags = (coef.cpu() != 0).tolist()
        ts, s0, s1, coef = (v.to(dev) for v in (ts, s0, s1, coef))
        ctx, ones = _guided_ctx(te, tok, dev), torch.ones(b, device=dev)
        xin, xt = ops.noisy_input(None, z, ones, ones, 2, BF16)
        history, x0_prev = [torch.empty_like(z), torch.empty_like(z)], None
        for i in range(N):
            assert not flags[i][3]                                           # deterministic: no noise term
            eps = unet.forward_nhwc(xin, ts[i].expand(2 * b).contiguous(), ctx, control=state)
            xin, xt, x0_prev = ops.solver_step(eps, xt, s0[i].expand(b).contiguous(), s1[i].expand(b).contiguous(), coef[i].expand(b, 4).contiguous(),
                                               kappa, BF16, prediction_type='epsilon', x0p=x0_prev if flags[i][2] else None, noise=None, scale=None,
                                               last=i == N - 1, x0_out=history[i & 1], need_prev=flags[i][2])
    torch.cuda.synchronize()
    assert torch.equal(got, xt)
    assert torch.isfinite(got).all() and not torch.equal(got, plain)


def test_sid_sd_sampler_with_control(dev):
    from sid_lsg_amd import ops
    from sid_lsg_amd.sd_util import encode_contexts, sid_sd_sampler
    unet, sched, te, tok, net, img = model(dev)
    z = _z(dev)
    init_t = torch.full((2,), 625, dtype=torch.long, device=dev)
    state = net.prepare(img, 1.0, dup=1)
    kw = dict(unet=unet, latents=z, contexts=PROMPTS, init_timesteps=init_t, noise_scheduler=sched, text_encoder=te, tokenizer=tok, resolution=64,
              train_sampler=False, num_steps_eval=2)
    torch.manual_seed(5)
    got = sid_sd_sampler(control=state, **kw)
    torch.manual_seed(5)
    plain = sid_sd_sampler(**kw)
    torch.manual_seed(5)
    with torch.no_grad():
        emb = encode_contexts(PROMPTS, te, tok, dev).to(BF16).contiguous()
        D = None
        for i in range(2):
            noise = z if i == 0 else torch.randn_like(z)
            t_i = (init_t * (1 - i / 2)).to(torch.long).contiguous()
            s0, s1 = sched.coefficients(t_i)
            xin, xt = ops.noisy_input(D, noise.to(F32).contiguous(), s0, s1, 1, BF16)
            eps = unet.forward_nhwc(xin, t_i, emb, control=state)
            D = ops.cfg_x0(eps, xt, s0, s1, 1.0, True, BF16, prediction_type='epsilon')
    torch.cuda.synchronize()
    assert torch.equal(got, D.to(F32))
    assert torch.isfinite(got).all() and not torch.equal(got, plain)
    with pytest.raises(ValueError, match='train_sampler=False'):
        sid_sd_sampler(**dict(kw, train_sampler=True, control=state))


# ---- 7. control composes with init_latents + mask -------------------------------------------------------------------------------------
def test_masked_sampling_with_control_keeps_the_known_region_exactly(dev):
    from sid_lsg_amd.sd_util import teacher_sample_i2i, teacher_sample_solver_i2i
    unet, sched, te, tok, net, img = model(dev)
    z, z0 = _z(dev), _z(dev, seed=12) * 0.5
    mask = torch.zeros(2, 8, 8, dtype=torch.uint8)
    mask[0, 2:6, 1:5] = 1
    mask[1, :, 4:] = 1
    mask = mask.to(dev)
    state = net.prepare(img, 1.0, dup=2)
    keep, paint = (mask == 0)[:, None].expand_as(z0), (mask != 0)[:, None].expand_as(z0)
    for fn, kw in ((teacher_sample_i2i, {}), (teacher_sample_solver_i2i, dict(solver='dpmpp2m'))):
        common = dict(guidance_scale=2.5, num_inference_steps=4, init_latents=z0, start_index=1, mask=mask, **kw)
        got = fn(unet, z, PROMPTS, sched, te, tok, 64, control=state, **common)
        plain = fn(unet, z, PROMPTS, sched, te, tok, 64, **common)
        torch.cuda.synchronize()
        assert torch.equal(got[keep], z0[keep]) and torch.equal(plain[keep], z0[keep])          # the exact bits of the known region
        assert torch.isfinite(got).all() and not torch.equal(got[paint], plain[paint])
        assert float((got[paint] - plain[paint]).abs().max()) > 1e-3


# ---- 8. command line ---------------------------------------------------------------------------------------------------------------------
def _png_pixels(path):
    import PIL.Image
    return np.asarray(PIL.Image.open(path).convert('RGB'))


def test_generate_onestep_with_a_controlnet(dev, tmp_path):
    """`generate_onestep.py --network teacher --controlnet random:controlnet --control_images DIR` in a child process, then the same command and
    the command without the three options in this process (as tests/test_gpu_cli.py runs the command): the PNGs exist, are identical across
    the two controlled runs and differ from the uncontrolled ones; stdout names the ControlNet and the scale."""
    import PIL.Image
    from click.testing import CliRunner
    import generate_onestep
    prompts = tmp_path / 'prompts.txt'
    prompts.write_text('a red cube\na blue sphere\n')
    ctl = tmp_path / 'ctl'
    ctl.mkdir()
    g = torch.Generator().manual_seed(2)
    for i in range(2):
        PIL.Image.fromarray(torch.randint(0, 256, (64, 64, 3), generator=g, dtype=torch.uint8).numpy()).save(str(ctl / f'edge{i}.png'))
    common = ['--network', 'teacher', '--repo_id', 'random:tiny', '--teacher_steps', '2', '--seeds', '0-1', '--resolution', '64',
              '--text_prompts', str(prompts)]
    control = ['--controlnet', 'random:controlnet', '--control_images', str(ctl), '--control_scale', '0.75']
    with socket.socket() as sock:           # a rendezvous port of the child's own: this process may hold the default one
        sock.bind(('127.0.0.1', 0))
        port = sock.getsockname()[1]
    out_a, out_b, out_p = tmp_path / 'a', tmp_path / 'b', tmp_path / 'plain'
    res = subprocess.run([sys.executable, os.path.join(ROOT, 'generate_onestep.py'), '--outdir', str(out_a)] + common + control,
                         cwd=ROOT, capture_output=True, text=True, timeout=240, env=dict(os.environ, MASTER_PORT=str(port)))
    assert res.returncode == 0, res.stdout + res.stderr
    assert 'ControlNet "random:controlnet": scale 0.75' in res.stdout
    r2 = CliRunner().invoke(generate_onestep.main, ['--outdir', str(out_b)] + common + control, catch_exceptions=False)
    assert r2.exit_code == 0 and 'ControlNet "random:controlnet": scale 0.75' in r2.output, r2.output
    r3 = CliRunner().invoke(generate_onestep.main, ['--outdir', str(out_p)] + common, catch_exceptions=False)
    assert r3.exit_code == 0 and 'ControlNet' not in r3.output, r3.output
    names = ['000000.png', '000001.png']
    pix = {}
    for d in (out_a, out_b, out_p):
        assert [os.path.basename(f) for f in sorted(glob.glob(str(d / '*.png')))] == names
        pix[d] = [_png_pixels(str(d / n)) for n in names]
    for a, b, p in zip(pix[out_a], pix[out_b], pix[out_p]):
        assert a.shape == (64, 64, 3) and a.min() != a.max()
        assert np.array_equal(a, b) and not np.array_equal(a, p)
