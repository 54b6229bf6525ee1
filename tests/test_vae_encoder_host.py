"""Host side of image-to-image generation: the VAE encoder's parameter names, the --strength mapping, the option refusals and the
init-image loader of generate_onestep.py, and the bottom/right-padded convolution of the restatement.  No GPU."""
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F


def test_encoder_keys_are_the_restatements():
    from sid_lsg_amd.vae import HipAutoencoderKLEncoder
    from vae_encoder_ref import VAE_CONFIGS, AutoencoderKLEncoderRef
    for arch in ('sd', 'tiny'):
        hip = HipAutoencoderKLEncoder(arch).init_parameters(seed=1)
        ref = AutoencoderKLEncoderRef(VAE_CONFIGS[arch])
        assert set(hip.state_dict()) == set(ref.state_dict())
        res = ref.load_state_dict(hip.state_dict(), strict=True)
        assert not res.missing_keys and not res.unexpected_keys
        for k, v in ref.state_dict().items():
            assert v.shape == hip.state_dict()[k].shape, k


# every parameter of a diffusers Stable Diffusion AutoencoderKL (block_out_channels 128/256/512/512, layers_per_block 2), by pattern
_RES = r'resnets\.[0-2]\.(norm1|norm2|conv1|conv2)\.(weight|bias)'
_MID = (r'mid_block\.(resnets\.[01]\.(norm1|norm2|conv1|conv2)|attentions\.0\.(group_norm|to_q|to_k|to_v|to_out\.0))\.(weight|bias)')
ENCODER_PATTERNS = [r'encoder\.conv_in\.(weight|bias)', r'encoder\.down_blocks\.[0-3]\.' + _RES.replace('[0-2]', '[01]'),
                    r'encoder\.down_blocks\.[12]\.resnets\.0\.conv_shortcut\.(weight|bias)',
                    r'encoder\.down_blocks\.[0-2]\.downsamplers\.0\.conv\.(weight|bias)', r'encoder\.' + _MID,
                    r'encoder\.conv_norm_out\.(weight|bias)', r'encoder\.conv_out\.(weight|bias)', r'quant_conv\.(weight|bias)']
DECODER_PATTERNS = [r'decoder\.conv_in\.(weight|bias)', r'decoder\.up_blocks\.[0-3]\.' + _RES,
                    r'decoder\.up_blocks\.[23]\.resnets\.0\.conv_shortcut\.(weight|bias)',
                    r'decoder\.up_blocks\.[0-2]\.upsamplers\.0\.conv\.(weight|bias)', r'decoder\.' + _MID,
                    r'decoder\.conv_norm_out\.(weight|bias)', r'decoder\.conv_out\.(weight|bias)', r'post_quant_conv\.(weight|bias)']
# parameter count of each half: 2 per conv / norm / linear
ENCODER_COUNT = 2 * (1 + 8 * 4 + 2 + 3 + (2 * 4 + 5) + 1 + 1 + 1)
DECODER_COUNT = 2 * (1 + 12 * 4 + 2 + 3 + (2 * 4 + 5) + 1 + 1 + 1)


def test_encoder_and_decoder_keys_partition_the_sd_vae():
    from sid_lsg_amd.vae import HipAutoencoderKLDecoder, HipAutoencoderKLEncoder
    enc, dec = set(HipAutoencoderKLEncoder('sd').state_dict()), set(HipAutoencoderKLDecoder('sd').state_dict())
    assert not enc & dec
    for keys, pats, count in ((enc, ENCODER_PATTERNS, ENCODER_COUNT), (dec, DECODER_PATTERNS, DECODER_COUNT)):
        for k in keys:
            assert sum(bool(re.fullmatch(p, k)) for p in pats) == 1, k
        assert len(keys) == count
    # a whole-VAE checkpoint loads into both halves, each ignoring the other's keys
    full = {k: torch.zeros(1) for k in enc | dec}
    e = HipAutoencoderKLEncoder('sd')
    assert set(k for k in full if k.startswith(('encoder.', 'quant_conv.'))) == enc
    with pytest.raises(RuntimeError):                      # shapes differ (zeros(1)): proves the encoder keys are really consumed
        e.load_state_dict(full)
    sd = HipAutoencoderKLEncoder('tiny').init_parameters(2).state_dict()
    sd.update({'decoder.conv_in.weight': torch.zeros(1), 'post_quant_conv.bias': torch.zeros(1)})
    res = HipAutoencoderKLEncoder('tiny').load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys


def test_strength_to_step_table():
    from generate_onestep import strength_to_step
    for s, k in ((1, 0), (0.75, 1), (0.6, 1), (0.5, 2), (0.25, 3), (0.01, 3)):
        assert strength_to_step(s, 4) == k, (s, k)
    for s in (1, 0.75, 0.5, 0.01):
        assert strength_to_step(s, 1) == 0
    assert strength_to_step(0.3, 10) == 7 and strength_to_step(0.5, 2) == 1 and strength_to_step(1.0, 2) == 0
    for bad in (0, -0.1, 1.5):
        with pytest.raises(ValueError):
            strength_to_step(bad, 4)


def _write_pngs(d):
    import PIL.Image
    rng = np.random.default_rng(0)
    imgs = {'b.png': rng.integers(0, 256, (16, 16, 3), dtype=np.uint8), 'a.png': rng.integers(0, 256, (16, 24, 3), dtype=np.uint8),
            'c.PNG': rng.integers(0, 256, (20, 16, 3), dtype=np.uint8)}
    for name, px in imgs.items():
        PIL.Image.fromarray(px, 'RGB').save(d / name)
    (d / 'notes.txt').write_text('not an image')
    return imgs


def test_init_image_loader(tmp_path):
    import generate_onestep as g
    imgs = _write_pngs(tmp_path)
    files = g.list_init_images(str(tmp_path))
    assert [f.rsplit('/', 1)[1] for f in files] == ['a.png', 'b.png', 'c.PNG']          # sorted by name, other files ignored
    batch = g.load_init_batch(files, [0, 1, 2, 3, 7], 16)
    assert batch.shape == (5, 16, 16, 3) and batch.dtype == np.uint8
    assert np.array_equal(batch[0], imgs['a.png'][:, 4:20])        # 16 x 24: the centre 16 columns, no resize
    assert np.array_equal(batch[1], imgs['b.png'])
    assert np.array_equal(batch[2], imgs['c.PNG'][2:18])           # 20 x 16: the centre 16 rows
    assert np.array_equal(batch[3], batch[0]) and np.array_equal(batch[4], batch[1])    # idx % len(files)
    import PIL.Image
    want = np.asarray(PIL.Image.fromarray(imgs['b.png'], 'RGB').resize((8, 8), PIL.Image.LANCZOS))
    assert np.array_equal(g.load_init_image(files[1], 8), want)


def test_click_refusals(tmp_path):
    from click.testing import CliRunner
    import generate_onestep as g
    run = lambda *a: CliRunner().invoke(g.main, ['--outdir', str(tmp_path / 'o'), '--repo_id', 'random:tiny', *a])  # noqa: E731
    r = run('--network', 'x.pkl', '--strength', '0.5')
    assert r.exit_code == 2 and '--strength' in r.output and '--init_images' in r.output
    r = run('--network', 'x.pkl', '--sample_posterior', '1')
    assert r.exit_code == 2 and '--sample_posterior' in r.output
    empty = tmp_path / 'empty'
    empty.mkdir()
    r = run('--network', 'x.pkl', '--init_images', str(empty))
    assert r.exit_code == 2 and 'no PNG or JPEG' in r.output
    _write_pngs(tmp_path)
    r = run('--network', 'teacher', '--init_images', str(tmp_path))
    assert r.exit_code == 2 and 'teacher' in r.output
    r = run('--network', 'x.pkl', '--init_images', str(tmp_path), '--strength', '0')
    assert r.exit_code == 2
    assert g.init_image_options('x.pkl', None, None, None, 4) is None
    files, k, sample = g.init_image_options('x.pkl', str(tmp_path), 0.5, None, 4)
    assert len(files) == 3 and k == 2 and sample is False


def test_restatement_downsample_pads_bottom_and_right():
    from vae_encoder_ref import downsample_br
    g = torch.Generator().manual_seed(0)
    x, w, b = torch.randn(2, 5, 6, 8, generator=g), torch.randn(7, 5, 3, 3, generator=g), torch.randn(7, generator=g)
    padded = torch.zeros(2, 5, 7, 9)
    padded[:, :, :6, :8] = x
    assert torch.equal(downsample_br(x, w, b), F.conv2d(padded, w, b, stride=2))
    assert downsample_br(x, w, b).shape == (2, 7, 3, 4)


def test_encoder_refuses_cpu_tensors():
    from sid_lsg_amd.vae import HipAutoencoderKLEncoder
    enc = HipAutoencoderKLEncoder('tiny').init_parameters(0)
    with pytest.raises(RuntimeError):
        enc.encode(torch.zeros(1, 3, 64, 64))
    with pytest.raises(RuntimeError):
        enc.encode_latents(torch.zeros(1, 64, 64, 3, dtype=torch.uint8))


def test_sampler_refuses_inconsistent_init_arguments():
    from sid_lsg_amd.sd_util import sid_sd_sampler
    z = torch.zeros(1, 4, 8, 8)
    with pytest.raises(ValueError):
        sid_sd_sampler(None, z, None, None, None, None, None, 64, train_sampler=True, init_latents=z)
    with pytest.raises(ValueError):
        sid_sd_sampler(None, z, None, None, None, None, None, 64, train_sampler=False, num_steps_eval=2, init_latents=z, start_step=2)
    with pytest.raises(ValueError):
        sid_sd_sampler(None, z, None, None, None, None, None, 64, train_sampler=False, start_step=1)
