"""Image-to-image generation on the GPU: the four kernels of AutoencoderKL.encode, HipAutoencoderKLEncoder against the fp32
restatement (tests/vae_encoder_ref.py), the sampler's init_latents / start_step and generate_onestep.py --init_images."""
import glob
import os
import pickle
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs an MI355X')
    from sid_lsg_amd._lib import lib
    lib.load()
    return torch.device('cuda:0')


def _rnd(*shape, seed=0, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(BF16)


# ---- stride-2 conv, bottom / right padding -------------------------------------------------------------------------------------------
def _conv_br_ref(x, w, bias=None):
    """fp32 F.pad(x, (0, 1, 0, 1)) + conv2d(stride 2, no padding) on the bf16-rounded operands; NHWC in and out."""
    cout, cin = w.shape[0], w.shape[1] // 9
    wn = w.float().view(cout, 3, 3, cin).permute(0, 3, 1, 2)
    y = F.conv2d(F.pad(x.float().permute(0, 3, 1, 2), (0, 1, 0, 1)), wn, bias, stride=2, padding=0)
    return y.permute(0, 2, 3, 1)


@pytest.mark.parametrize('H,W', [(4, 6), (16, 8)])
@pytest.mark.parametrize('Cin,Cout', [(32, 32), (128, 128), (64, 128)])
def test_conv3x3_bottom_right_padding(dev, H, W, Cin, Cout):
    """Bounds: those of test_gpu_ops.py::test_conv3x3 for its stride-2 cases (2e-3 on the fp32 output, 1.2e-2 on the bf16 output with
    its epilogue)."""
    from sid_lsg_amd import ops
    from test_gpu_ops import close
    B = 2
    x, w = _rnd(B, H, W, Cin, seed=1), _rnd(Cout, 9 * Cin, seed=2, scale=(9 * Cin) ** -0.5)
    ref = _conv_br_ref(x, w)
    assert ref.shape == (B, H // 2, W // 2, Cout)
    close(ops.conv3x3(x.to(dev), w.to(dev), stride=2, pad='br', out_f32=True), ref, 2e-3, 'conv br')
    bias = torch.randn(Cout, generator=torch.Generator().manual_seed(3))
    got = ops.conv3x3(x.to(dev), w.to(dev), bias=bias.to(dev), stride=2, pad='br')
    assert got.dtype == BF16
    close(got, ref + bias, 1.2e-2, 'conv br + bias')
    # which side is padded: an input that lives on the first row / column only, and one on the last row / column only, must light up
    # exactly the outputs the reference lights up (symmetric padding, or padding on the top / left, moves them)
    for name, rows, cols in (('first', 0, 0), ('last', H - 1, W - 1)):
        xe = torch.zeros_like(x)
        xe[:, rows] = x[:, rows]
        xe[:, :, cols] = x[:, :, cols]
        want = _conv_br_ref(xe, w)
        out = ops.conv3x3(xe.to(dev), w.to(dev), stride=2, pad='br', out_f32=True).cpu()
        assert torch.equal(out != 0, want != 0), name
        assert (want != 0).any() and not (want != 0).all()
        close(out, want, 2e-3, f'conv br {name} row / column')
    # and it is not the symmetric stride-2 conv
    sym = ops.conv3x3(x.to(dev), w.to(dev), stride=2, out_f32=True).cpu()
    assert (sym - ref).abs().max() > 0.05 * ref.abs().max()


def test_conv3x3_bottom_right_refuses_odd_sizes(dev):
    from sid_lsg_amd import ops
    from sid_lsg_amd._lib import lib
    x, w = _rnd(1, 5, 6, 32, seed=1).to(dev), _rnd(32, 9 * 32, seed=2).to(dev)
    out = torch.empty((1, 3, 3, 32), device=dev, dtype=BF16)
    s = torch.cuda.current_stream().cuda_stream
    assert lib.sidlsg_conv3x3_br_bf16.raw(x.data_ptr(), 32, w.data_ptr(), out.data_ptr(), 32, None, 1, 5, 6, 32, 32, 0, s) == -22
    assert lib.sidlsg_conv3x3_br_bf16.raw(x.data_ptr(), 32, w.data_ptr(), out.data_ptr(), 32, None, 1, 6, 5, 32, 32, 0, s) == -22
    with pytest.raises(RuntimeError):
        ops.conv3x3(x, w, stride=2, pad='br')
    with pytest.raises(RuntimeError):
        ops.conv3x3(x[:, :4], w, stride=1, pad='br')


# ---- wide attention ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,N', [(2, 64), (1, 144), (1, 1040)])
def test_wide_attention(dev, B, N):
    """One head of width 512 against the fp32 softmax reference on the bf16-rounded operands, at the forward bound of
    test_gpu_ops.py::test_self_attention.  N = 144 and 1040 end in a half key tile (N % 32 == 16); 144 leaves three idle waves in the
    last block; q, k, v are column slices of one fused [B, N, 1536] buffer, as the encoder passes them."""
    from sid_lsg_amd import ops
    from test_gpu_ops import attn_ref, close
    D = 512
    qkv = _rnd(B, N, 3 * D, seed=1)
    ref = attn_ref(qkv[..., :D].float(), qkv[..., D:2 * D].float(), qkv[..., 2 * D:].float(), 1)
    qd = qkv.to(dev)
    got = ops.wide_attention(qd[..., :D], qd[..., D:2 * D], qd[..., 2 * D:])
    assert got.dtype == BF16 and got.shape == (B, N, D)
    close(got, ref, 1.2e-2, 'wide attention')
    q, k, v = (qkv[..., i * D:(i + 1) * D].contiguous().to(dev) for i in range(3))
    assert torch.equal(ops.wide_attention(q, k, v), got)            # contiguous operands: the same bits


@pytest.mark.parametrize('N', [144, 1040])
def test_wide_attention_rescales_when_the_maximum_rises(dev, N):
    """Keys ordered so that every query's logit grows with the key index, from -40 g to +40 g (g in [0.5, 1] per query): the running
    maximum of every row rises in every 32-key tile, by up to 80 / (N / 32) per tile, and the weight sits on the last keys.  A kernel
    that misses a rescale keeps the early tiles' e^(+40 ..) weights (or overflows); one that rescales with a stale factor loses the
    row.  Same bound as above; the output must be finite."""
    from sid_lsg_amd import ops
    from test_gpu_ops import attn_ref, close
    D = 512
    g = torch.Generator().manual_seed(7)
    gain = 0.5 + 0.5 * torch.rand(N, 1, generator=g)
    ramp = torch.linspace(-40.0, 40.0, N)[:, None]
    q = (gain * torch.ones(N, D) + 0.05 * torch.randn(N, D, generator=g)).to(BF16)[None]
    k = (ramp * D ** -0.5 * torch.ones(N, D) + 0.05 * torch.randn(N, D, generator=g)).to(BF16)[None]
    v = torch.randn(1, N, D, generator=g).to(BF16)
    logits = q[0].float() @ k[0].float().t() * D ** -0.5
    assert logits.max() > 30 and logits.min() < -30
    tile_max = logits[:, :N // 32 * 32].view(N, -1, 32).max(-1).values
    assert (tile_max[:, 1:] > tile_max[:, :-1]).float().mean() > 0.9          # the premise: the maximum rises tile after tile
    ref = attn_ref(q.float(), k.float(), v.float(), 1)
    got = ops.wide_attention(q.to(dev), k.to(dev), v.to(dev))
    assert bool(torch.isfinite(got).all())
    close(got, ref, 1.2e-2, 'forced rescale')
    # the mirror image (maximum in the first tile, never rising again) through the same kernel
    got_r = ops.wide_attention(q.to(dev), k.flip(1).contiguous().to(dev), v.flip(1).contiguous().to(dev))
    close(got_r, ref, 1.2e-2, 'maximum first')


def test_wide_attention_refuses_other_widths(dev):
    from sid_lsg_amd import ops
    from sid_lsg_amd._lib import lib
    q = _rnd(1, 64, 256).to(dev)
    o = torch.empty_like(q)
    s = torch.cuda.current_stream().cuda_stream
    p = q.data_ptr()
    assert lib.sidlsg_attn_fwd_wide.raw(p, p, p, o.data_ptr(), 1, 64, 256, 256, 256, 256, 256, 64 * 256, 64 * 256, 64 * 256, 64 * 256, s) == -22
    with pytest.raises(RuntimeError):
        ops.wide_attention(q, q, q)
    x = _rnd(1, 40, 512).to(dev)                                      # N not a multiple of 16
    with pytest.raises(RuntimeError):
        ops.wide_attention(x, x, x)


# ---- image conversion and posterior --------------------------------------------------------------------------------------------------
def test_image_to_nhwc8_is_bit_exact(dev):
    """uint8: every byte value, against x / 127.5 - 1 evaluated in fp32 on the host (IEEE division, then subtraction) and rounded to
    bf16; fp32 NCHW: against the rounding of the input.  Channels 3..7 are zero."""
    from sid_lsg_amd import ops
    u8 = torch.arange(2 * 8 * 16 * 3, dtype=torch.int64).remainder(256).to(torch.uint8).view(2, 8, 16, 3)
    u8[1] = torch.randint(0, 256, (8, 16, 3), generator=torch.Generator().manual_seed(0), dtype=torch.uint8)
    got = ops.image_to_nhwc8(u8.to(dev)).cpu()
    want = torch.zeros(2, 8, 16, 8, dtype=BF16)
    want[..., :3] = (u8.to(F32) / 127.5 - 1).to(BF16)
    assert got.dtype == BF16 and torch.equal(got.view(torch.int16), want.view(torch.int16))
    f = torch.rand(2, 3, 8, 16, generator=torch.Generator().manual_seed(1)) * 2 - 1
    got = ops.image_to_nhwc8(f.to(dev)).cpu()
    want = torch.zeros(2, 8, 16, 8, dtype=BF16)
    want[..., :3] = f.permute(0, 2, 3, 1).to(BF16)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    with pytest.raises(RuntimeError):
        ops.image_to_nhwc8(u8.permute(0, 3, 1, 2).contiguous().to(dev))


@pytest.mark.parametrize('with_eps', [True, False])
def test_vae_posterior(dev, with_eps):
    """Against the torch expression in fp32: conv2d 1x1, chunk, clamp(-30, 20), exp(0.5 logvar), mean + std eps, times the scaling
    factor.  rtol 1e-5; the absolute term covers cancellation inside the 8-term dot products: 8 roundings of 2^-23 relative to the
    largest sum of |w y| + |b| (times the scaling factor, plus std |eps|, for z).  Moments beyond both clamp ends are fed."""
    from sid_lsg_amd import ops
    g = torch.Generator().manual_seed(3)
    B, h, w, sf = 2, 5, 7, 0.18215
    mom = torch.randn(B, h, w, 8, generator=g)
    mom[..., 4:] = mom[..., 4:] * 30                                   # logvar well past -30 and +20
    qw = torch.eye(8) + 0.1 * torch.randn(8, 8, generator=g)
    qb = 0.1 * torch.randn(8, generator=g)
    eps = torch.randn(B, 4, h, w, generator=g) if with_eps else None
    m = F.conv2d(mom.permute(0, 3, 1, 2), qw.view(8, 8, 1, 1), qb)
    mean, logvar = m.chunk(2, dim=1)
    assert logvar.max() > 25 and logvar.min() < -35
    logvar = logvar.clamp(-30.0, 20.0)
    std = torch.exp(0.5 * logvar)
    z = (mean + std * eps if with_eps else mean) * sf
    amax = float((mom.abs() @ qw.abs().t() + qb.abs()).max())
    atol = 2.0 ** -20 * amax
    gz, gm, gl = ops.vae_posterior(mom.to(dev), qw.to(dev), qb.to(dev), sf, eps=eps.to(dev) if with_eps else None, want_moments=True)
    torch.testing.assert_close(gm.cpu(), mean, rtol=1e-5, atol=atol)
    torch.testing.assert_close(gl.cpu(), logvar, rtol=1e-5, atol=atol)
    assert float(gl.max()) == 20.0 and float(gl.min()) == -30.0
    torch.testing.assert_close(gz.cpu(), z, rtol=1e-5, atol=sf * atol)
    only_z = ops.vae_posterior(mom.to(dev), qw.to(dev), qb.to(dev), sf, eps=eps.to(dev) if with_eps else None)
    assert torch.equal(only_z, gz)


# ---- the encoder ---------------------------------------------------------------------------------------------------------------------
def _pair(arch, seed=3):
    """(HIP encoder, restatement) with equal weights, matmul weights bf16-representable on both sides (as tests/test_gpu_vae.py)."""
    from sid_lsg_amd.vae import HipAutoencoderKLEncoder
    from vae_encoder_ref import VAE_CONFIGS, AutoencoderKLEncoderRef
    hip = HipAutoencoderKLEncoder(arch).init_parameters(seed=seed)
    ref = AutoencoderKLEncoderRef(VAE_CONFIGS[arch]).requires_grad_(False)
    res = ref.load_state_dict(hip.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    with torch.no_grad():
        for _, p in ref.named_parameters():
            if p.ndim >= 2:
                p.copy_(p.to(BF16).float())
    hip.load_state_dict(ref.state_dict())
    return hip, ref


def _rel(got, want):
    return (got.float().cpu() - want).abs().max().item() / want.abs().max().item()


@pytest.mark.parametrize('res', [64, 96])
def test_encoder_matches_restatement(dev, res):
    hip, ref = _pair('tiny')
    hip = hip.to(dev)
    lat, sf = res // 8, hip.config.scaling_factor
    u8 = torch.randint(0, 256, (2, res, res, 3), generator=torch.Generator().manual_seed(0), dtype=torch.uint8)
    want = ref.encode((u8.to(F32) / 127.5 - 1).permute(0, 3, 1, 2).contiguous())
    dist = hip.encode(u8.to(dev)).latent_dist
    for t in (dist.mean, dist.logvar, dist.std, dist.var, dist.mode()):
        assert t.shape == (2, 4, lat, lat) and t.dtype == F32
    errs = dict(mean=_rel(dist.mean, want.mean), logvar=_rel(dist.logvar, want.logvar), mode=_rel(hip.encode_latents(u8.to(dev)), want.mode() * sf))
    print(f'vae encode {res}: rel max err {errs}')
    assert max(errs.values()) < 4e-2          # the decoder test's bound: bf16 activations through as many conv layers vs fp32
    assert float(dist.logvar.max()) <= 20.0 and float(dist.logvar.min()) >= -30.0
    assert torch.equal(dist.std, torch.exp(0.5 * dist.logvar))
    # sampling: a given eps through the kernel, through the distribution object, and by hand from the HIP moments
    eps = torch.randn(2, 4, lat, lat, generator=torch.Generator().manual_seed(1)).to(dev)
    by_hand = dist.mean + dist.std * eps
    torch.testing.assert_close(dist.sample(eps=eps), by_hand, rtol=0, atol=0)
    torch.testing.assert_close(hip.encode_latents(u8.to(dev), eps=eps), by_hand * sf, rtol=1e-6, atol=1e-6 * float(by_hand.abs().max()) * sf)
    gen = torch.Generator(dev).manual_seed(5)
    s1 = dist.sample(generator=gen)
    assert s1.shape == by_hand.shape and not torch.equal(s1, dist.mean)
    # fp32 NCHW images in [-1, 1] holding the same values: the same bits
    same = hip.encode((u8.to(F32) / 127.5 - 1).permute(0, 3, 1, 2).contiguous().to(dev), return_dict=False)[0]
    assert torch.equal(same.mean, dist.mean) and torch.equal(same.logvar, dist.logvar)
    with pytest.raises(RuntimeError):
        hip.encode(u8[:, :60].contiguous().to(dev))


def test_sd_encoder_one_pass_through_wide_attention(dev, monkeypatch):
    """The `sd` architecture at 64 x 64: 8 x 8 latents, 64 tokens of width 512 in the mid block."""
    from sid_lsg_amd import ops
    hip, ref = _pair('sd', seed=4)
    hip = hip.to(dev)
    calls = []
    real = ops.wide_attention
    monkeypatch.setattr(ops, 'wide_attention', lambda q, k, v: calls.append(tuple(q.shape)) or real(q, k, v))
    monkeypatch.setattr(F, 'scaled_dot_product_attention', lambda *a, **k: pytest.fail('SDPA on the encoder path'))
    x = torch.rand(1, 3, 64, 64, generator=torch.Generator().manual_seed(2)) * 2 - 1
    want = ref.encode(x)
    dist = hip.encode(x.to(dev)).latent_dist
    assert calls == [(1, 64, 512)]
    assert dist.mean.shape == (1, 4, 8, 8)
    errs = dict(mean=_rel(dist.mean, want.mean), logvar=_rel(dist.logvar, want.logvar))
    print(f'sd vae encode 64: rel max err {errs}')
    assert max(errs.values()) < 4e-2


# ---- sampler -------------------------------------------------------------------------------------------------------------------------
PROMPTS = ['a red cube on a table', 'two blue spheres']


def test_sampler_enters_the_chain_at_start_step(dev):
    from sid_lsg_amd.sd_util import encode_contexts, hip_generate, load_sd15, sid_sd_sampler, step_timesteps
    unet, _, sched, te, tok = load_sd15('random:tiny', None, dev, F32)
    unet.eval().requires_grad_(False)
    g = torch.Generator().manual_seed(11)
    z, L = torch.randn(2, 4, 8, 8, generator=g).to(dev), (0.5 * torch.randn(2, 4, 8, 8, generator=g)).to(dev)
    t0 = 625 * torch.ones(2, device=dev, dtype=torch.long)
    kw = dict(unet=unet, latents=z, contexts=PROMPTS, init_timesteps=t0, noise_scheduler=sched, text_encoder=te, tokenizer=tok, resolution=64,
              train_sampler=False, num_steps_eval=4)
    torch.manual_seed(5)
    got = sid_sd_sampler(init_latents=L, start_step=2, **kw)
    torch.manual_seed(5)
    with torch.no_grad():
        emb = encode_contexts(PROMPTS, te, tok, dev).to(unet.compute_dtype).contiguous()
        ts = step_timesteps(t0, 4)
        x = hip_generate(unet, z, emb, ts[2].contiguous(), sched, x0=L)
        x = hip_generate(unet, torch.randn_like(z), emb, ts[3].contiguous(), sched, x0=x)
    assert got.dtype == F32 and torch.equal(got, x)
    # the defaults are today's call
    torch.manual_seed(5)
    a = sid_sd_sampler(**kw)
    torch.manual_seed(5)
    b = sid_sd_sampler(init_latents=None, start_step=0, **kw)
    assert torch.equal(a, b) and not torch.equal(a, got)
    # entering at the last step consumes no noise beyond z
    torch.manual_seed(5)
    last = sid_sd_sampler(init_latents=L, start_step=3, **kw)
    with torch.no_grad():
        assert torch.equal(last, hip_generate(unet, z, emb, ts[3].contiguous(), sched, x0=L))


# ---- command line --------------------------------------------------------------------------------------------------------------------
def _png_pixels(path):
    import PIL.Image
    return np.asarray(PIL.Image.open(path).convert('RGB'))


def _run_cli(args, out):
    with socket.socket() as sock:           # a rendezvous port of the child's own: this process may hold the default one
        sock.bind(('127.0.0.1', 0))
        port = sock.getsockname()[1]
    res = subprocess.run([sys.executable, os.path.join(ROOT, 'generate_onestep.py'), '--outdir', str(out)] + args, cwd=ROOT, capture_output=True,
                         text=True, timeout=240, env=dict(os.environ, MASTER_PORT=str(port)))
    assert res.returncode == 0, res.stdout + res.stderr
    files = sorted(glob.glob(str(out) + '_numstep2/*.png'))
    assert [os.path.basename(f) for f in files] == [f'{i:06d}.png' for i in range(4)]
    return [_png_pixels(f) for f in files], res.stdout


def test_generate_onestep_from_init_images(dev, tmp_path):
    import PIL.Image
    from sid_lsg_amd.sd_util import load_sd15, sid_sd_sampler
    unet = load_sd15('random:tiny', None, dev, F32, seed=7)[0]
    snap = tmp_path / 'network-snapshot.pkl'
    with open(snap, 'wb') as f:
        pickle.dump(dict(ema=unet), f)
    prompts = tmp_path / 'prompts.txt'
    prompts.write_text('a red cube\na blue sphere\nthree green cones\n')
    imgs = tmp_path / 'init'
    imgs.mkdir()
    rng = np.random.default_rng(0)
    for name, shape in (('b.png', (64, 64, 3)), ('a.png', (80, 100, 3))):
        PIL.Image.fromarray(rng.integers(0, 256, shape, dtype=np.uint8), 'RGB').save(imgs / name)
    common = ['--network', str(snap), '--repo_id', 'random:tiny', '--resolution', '64', '--num_steps_eval', '2', '--seeds', '0-3',
              '--text_prompts', str(prompts)]
    plain, _ = _run_cli(common, tmp_path / 'plain')
    i2i = ['--strength', '0.5', '--init_images', str(imgs)]
    first, log = _run_cli(common + i2i, tmp_path / 'i2i_a')
    second, _ = _run_cli(common + i2i, tmp_path / 'i2i_b')
    assert '2 init images' in log and 'entering at step 1 of 2' in log
    for a, b, p in zip(first, second, plain):
        assert a.shape == (64, 64, 3) and a.min() != a.max()
        assert np.array_equal(a, b) and not np.array_equal(a, p)
    # samples 0 and 2 start from the same file (idx % 2) but have their own z and prompt
    assert not np.array_equal(first[0], first[2])
    # without the option the script is the parent's: at one step (no noise beyond the per-seed z) its files hold exactly the pixels of
    # the sampler called the way the parent calls it
    from click.testing import CliRunner
    import generate_onestep
    out1 = tmp_path / 'one_step'
    r = CliRunner().invoke(generate_onestep.main, ['--outdir', str(out1), '--network', str(snap), '--repo_id', 'random:tiny', '--resolution', '64',
                                                   '--seeds', '0-3', '--text_prompts', str(prompts)], catch_exceptions=False)
    assert r.exit_code == 0, r.output
    with open(snap, 'rb') as f:
        G = pickle.load(f)['ema'].to(dev)
    G.eval().requires_grad_(False)
    _, vae, sched, te, tok = load_sd15('random:tiny', 'random:tiny', dev, BF16)
    z = generate_onestep.StackedRandomGenerator(dev, [0, 1, 2, 3]).randn([4, 4, 8, 8], device=dev)
    caps = ['a red cube', 'a blue sphere', 'three green cones']
    with torch.no_grad():
        images = sid_sd_sampler(unet=G, latents=z, contexts=[caps[i % 3] for i in range(4)],
                                init_timesteps=625 * torch.ones(4, device=dev, dtype=torch.long), noise_scheduler=sched, text_encoder=te,
                                tokenizer=tok, resolution=64, dtype=BF16, return_images=True, vae=vae, num_steps=1, train_sampler=False,
                                num_steps_eval=1)
    arr = (images.float() * 127.5 + 128).clip(0, 255).to(torch.uint8).permute(0, 2, 3, 1).cpu().numpy()
    for i in range(4):
        assert np.array_equal(_png_pixels(str(out1 / f'{i:06d}.png')), arr[i])
