"""v-prediction (SD 2.x 768-v) teachers, host side: the scheduler's config handling and closed forms, the loader's
scheduler resolution, and the v goldens (tools/make_vpred_goldens.py).  CPU only."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import fixtures
from sid_lsg_amd.scheduler import DDPMScheduler, prediction_mode

SD21_V = {'_class_name': 'DDIMScheduler', '_diffusers_version': '0.8.0', 'beta_end': 0.012, 'beta_schedule': 'scaled_linear',
          'beta_start': 0.00085, 'clip_sample': False, 'num_train_timesteps': 1000, 'prediction_type': 'v_prediction',
          'set_alpha_to_one': False, 'skip_prk_steps': True, 'steps_offset': 1, 'trained_betas': None}
SD15 = {'_class_name': 'PNDMScheduler', 'beta_end': 0.012, 'beta_schedule': 'scaled_linear', 'beta_start': 0.00085,
        'num_train_timesteps': 1000, 'set_alpha_to_one': False, 'skip_prk_steps': True, 'steps_offset': 1, 'timestep_spacing': 'leading'}


def _abar64(beta_start=0.00085, beta_end=0.012, n=1000, schedule='scaled_linear'):
    if schedule == 'scaled_linear':
        betas = np.linspace(beta_start ** 0.5, beta_end ** 0.5, n) ** 2
    else:
        betas = np.linspace(beta_start, beta_end, n)
    return np.cumprod(1.0 - betas)


def test_from_config_accepts_what_it_reproduces():
    s = DDPMScheduler.from_config(SD21_V)
    assert s.config.prediction_type == 'v_prediction' and s.mode == 2
    assert torch.equal(s.alphas_cumprod, DDPMScheduler().alphas_cumprod)          # the SD 2.x table is the SD 1.x one
    e = DDPMScheduler.from_config(SD15)
    assert e.config.prediction_type == 'epsilon' and e.mode == 1
    lin = DDPMScheduler.from_config(dict(beta_schedule='linear', beta_start=1e-4, beta_end=0.02, num_train_timesteps=500,
                                         prediction_type='epsilon', clip_sample=False))
    assert lin.alphas_cumprod.shape == (500,)
    np.testing.assert_allclose(lin.alphas_cumprod.double().numpy(), _abar64(1e-4, 0.02, 500, 'linear'), rtol=2e-6)


@pytest.mark.parametrize('change', [dict(trained_betas=[0.1] * 1000), dict(clip_sample=True), dict(thresholding=True),
                                    dict(rescale_betas_zero_snr=True), dict(prediction_type='sample'),
                                    dict(beta_schedule='squaredcos_cap_v2')])
def test_from_config_rejects_what_it_would_not_reproduce(change):
    with pytest.raises(ValueError):
        DDPMScheduler.from_config(dict(SD21_V, **change))


def test_unknown_prediction_type_raises():
    with pytest.raises(ValueError):
        DDPMScheduler(prediction_type='sample')
    with pytest.raises(ValueError):
        prediction_mode('sample')
    assert prediction_mode('epsilon') == 1 and prediction_mode('v_prediction') == 2


def test_v_step_velocity_and_snr_weight_match_float64_closed_forms():
    s = DDPMScheduler(prediction_type='v_prediction')
    ab = _abar64()
    g = torch.Generator().manual_seed(0)
    t = torch.tensor([20, 301, 625, 979])
    x0, noise, o = (torch.randn(4, 4, 8, 8, generator=g) for _ in range(3))
    a = torch.from_numpy(ab[t.numpy()]).view(-1, 1, 1, 1)
    s0, s1 = a.sqrt(), (1 - a).sqrt()
    xt = s.add_noise(x0, noise, t)
    np.testing.assert_allclose(xt.double().numpy(), (s0 * x0.double() + s1 * noise.double()).numpy(), rtol=1e-5, atol=1e-6)
    v = s.get_velocity(x0, noise, t)
    np.testing.assert_allclose(v.double().numpy(), (s0 * noise.double() - s1 * x0.double()).numpy(), rtol=1e-5, atol=1e-6)
    x0p = s.step(o, t, xt).pred_original_sample
    np.testing.assert_allclose(x0p.double().numpy(), (s0 * xt.double() - s1 * o.double()).numpy(), rtol=1e-5, atol=1e-6)
    # with the true velocity as the network output, the v step recovers x0
    np.testing.assert_allclose(s.step(v, t, xt).pred_original_sample.numpy(), x0.numpy(), atol=2e-5)
    # one scalar timestep (the sampler's form, init_timesteps[0])
    one = s.step(o[:1], torch.tensor(625), xt[:1]).pred_original_sample
    np.testing.assert_allclose(one.double().numpy(), (s0[2:3] * xt[:1].double() - s1[2:3] * o[:1].double()).numpy(), rtol=1e-5, atol=1e-6)
    snr = ab / (1 - ab)
    np.testing.assert_allclose(s.snr_weights(t).double().numpy(), (snr / (snr + 1))[t.numpy()], rtol=1e-6)
    # the weight is taken from abar exactly as compute_snr does (float32 abar / (1 - abar)), not from s0**2
    ac = s.alphas_cumprod[t]
    assert torch.equal(s.snr_weights(t), (ac / (1 - ac)) / (ac / (1 - ac) + 1))
    # the epsilon step is unchanged
    e = DDPMScheduler()
    np.testing.assert_allclose(e.step(o, t, xt).pred_original_sample.double().numpy(),
                               ((xt.double() - s1 * o.double()) / s0).numpy(), rtol=1e-4, atol=1e-5)


def test_scheduler_resolution_of_a_diffusers_directory(tmp_path, monkeypatch):
    """load_sd15 resolves its scheduler through sd_util.resolve_scheduler: a local diffusers-layout directory with a v
    scheduler_config.json (the stable-diffusion-2-1 checkpoint's) yields a v scheduler; without the file, today's default."""
    from sid_lsg_amd.sd_util import _arch_of, resolve_scheduler
    d = tmp_path / 'stable-diffusion-2-1'
    (d / 'scheduler').mkdir(parents=True)
    (d / 'scheduler' / 'scheduler_config.json').write_text(json.dumps(SD21_V))
    assert resolve_scheduler(str(d)).config.prediction_type == 'v_prediction'
    (d / 'scheduler' / 'scheduler_config.json').write_text(json.dumps(dict(SD21_V, clip_sample=True)))
    with pytest.raises(ValueError):
        resolve_scheduler(str(d))
    (d / 'scheduler' / 'scheduler_config.json').unlink()
    assert resolve_scheduler(str(d)).config.prediction_type == 'epsilon'
    # random specs
    assert resolve_scheduler('random:tiny:v').config.prediction_type == 'v_prediction'
    assert resolve_scheduler('random:tiny').config.prediction_type == 'epsilon'
    assert _arch_of('random:sd21-base:v') == 'sd21-base' and _arch_of('random:tiny:v') == 'tiny'
    with pytest.raises(ValueError):
        _arch_of('random:tiny:x')
    # hub ids: only with random init allowed, and only the 768-v ids (no '-base')
    monkeypatch.setenv('SIDLSG_ALLOW_RANDOM_INIT', '1')
    for hub, pt in (('stabilityai/stable-diffusion-2-1', 'v_prediction'), ('stabilityai/stable-diffusion-2', 'v_prediction'),
                    ('stabilityai/stable-diffusion-2-1-base', 'epsilon'), ('stabilityai/stable-diffusion-2-base', 'epsilon'),
                    ('runwayml/stable-diffusion-v1-5', 'epsilon')):
        assert resolve_scheduler(hub).config.prediction_type == pt, hub
        assert _arch_of(hub) == ('sd15' if 'v1-5' in hub else 'sd21-base')
    monkeypatch.setenv('SIDLSG_ALLOW_RANDOM_INIT', '0')
    assert resolve_scheduler('stabilityai/stable-diffusion-2-1').config.prediction_type == 'epsilon'


def test_network_parameterisation_travels_with_copies_and_snapshots():
    import pickle
    from sid_lsg_amd.sd_util import check_prediction_type
    from sid_lsg_amd.unet import CONFIGS, HipUNet2DCondition
    net = HipUNet2DCondition(CONFIGS['tiny'])
    assert net.prediction_type == 'epsilon'
    # snapshot state as __getstate__ writes it (weights omitted: the network is not materialised on the CPU)
    st = dict(cfg=CONFIGS['tiny'], state={}, training=False, compute_dtype=torch.bfloat16, prediction_type='v_prediction')
    back = HipUNet2DCondition.__new__(HipUNet2DCondition)
    back.__setstate__(pickle.loads(pickle.dumps(st)))
    assert back.prediction_type == 'v_prediction'
    del st['prediction_type']                      # a snapshot written before the attribute existed
    old = HipUNet2DCondition.__new__(HipUNet2DCondition)
    old.__setstate__(st)
    assert old.prediction_type == 'epsilon'
    check_prediction_type(back, DDPMScheduler(prediction_type='v_prediction'))
    with pytest.raises(ValueError):
        check_prediction_type(back, DDPMScheduler())
    with pytest.raises(ValueError):
        check_prediction_type(old, DDPMScheduler(prediction_type='v_prediction'))


@pytest.mark.parametrize('name', ['k15_a1', 'k1_a12'])
def test_v_loop_goldens_are_well_formed(golden_dir, name):
    g = np.load(os.path.join(golden_dir, f'loop_v_{name}.npz'))
    assert str(g['prediction_type']) == 'v_prediction' and str(g['cfg']) == 'tiny'
    np.testing.assert_allclose(np.array(fixtures.checksum(fixtures.make_unet('tiny'))), g['weight_checksum'], rtol=1e-12)
    it = int(g['kw_iterations'])
    assert [str(n) for n in g['loss_names']] == ['fake_score_Loss/loss', 'G_Loss/loss'] * it
    assert np.all(np.isfinite(g['loss_values'])) and np.all(g['loss_values'][0::2] > 0)
    # made with the unmodified reference loop: its v weighting is only per-sample at batch_gpu 1
    assert int(g['kw_batch_gpu']) == 1 and int(g['kw_batch_size']) >= 2
    for k in ('G_conv_in_w', 'fake_conv_in_w', 'G_last_b', 'fake_last_b'):
        assert np.all(np.isfinite(g[k]))


def test_v_glue_golden_is_well_formed(golden_dir):
    g = np.load(os.path.join(golden_dir, 'glue_v_tiny.npz'))
    assert str(g['prediction_type']) == 'v_prediction'
    np.testing.assert_allclose(np.array(fixtures.checksum(fixtures.make_unet('tiny'))), g['weight_checksum'], rtol=1e-12)
    np.testing.assert_allclose(np.array(fixtures.checksum(fixtures.make_unet('tiny', seed=99))), g['weight_checksum2'], rtol=1e-12)
    for b in (1, 2):
        assert g[f'b{b}_xhat'].shape == (b, 4, 8, 8)
        for kappa in (1.0, 2.0):
            for px0 in (0, 1):
                assert g[f'b{b}_k{kappa}_x0{px0}'].shape == (b, 4, 8, 8)
                assert np.all(np.isfinite(g[f'b{b}_k{kappa}_x0{px0}']))


def test_v_glue_golden_replays_through_the_v_closed_forms(golden_dir):
    """The reference's x0 under the v scheduler equals s0 x_t - s1 v of its raw (guided) output: the two stored branches of
    every case are tied together by the scheduler's own formulas (float64)."""
    g = np.load(os.path.join(golden_dir, 'glue_v_tiny.npz'))
    ab = _abar64()
    for b in (1, 2):
        t = g[f'b{b}_t']
        a = ab[t].reshape(-1, 1, 1, 1)
        xt = np.sqrt(a) * g[f'b{b}_xhat'].astype(np.float64) + np.sqrt(1 - a) * g[f'b{b}_noise'].astype(np.float64)
        for kappa in (1.0, 2.0):
            raw = g[f'b{b}_k{kappa}_x0{0}'].astype(np.float64)
            np.testing.assert_allclose(g[f'b{b}_k{kappa}_x0{1}'], np.sqrt(a) * xt - np.sqrt(1 - a) * raw, rtol=1e-4, atol=2e-5)


def test_v_fullsize_golden_is_well_formed(golden_dir):
    from oracle.unet_ref import CONFIGS, UNet2DConditionRef
    fx = np.load(os.path.join(golden_dir, 'fullsize_sd21v_k2_512.npz'))
    assert [str(v) for v in fx['case']] == ['sd21-base', '64', '1', '2.0', str(fixtures.FULLSIZE_LR)]
    assert str(fx['prediction_type']) == 'v_prediction'
    assert np.isfinite(float(fx['loss_fake'])) and np.isfinite(float(fx['loss_G'])) and float(fx['loss_fake']) > 0
    with torch.device('meta'):
        net = UNet2DConditionRef(CONFIGS['sd21-base'])
    n = sum(int(fixtures.sample_index(p.numel()).numel()) for p in net.parameters())
    shapes = {k: tuple(p.shape) for k, p in net.named_parameters()}
    for name in ('fake_score', 'G'):
        assert int(fx[name + '/n']) == n
        assert fx[name + '/sign'].shape == fx[name + '/big'].shape == ((n + 7) // 8,)
        assert np.unpackbits(fx[name + '/big'])[:n].mean() > 0.999
    for k in fixtures.FULLSIZE_EMA_NAMES:
        assert tuple(fx['ema/' + k].shape) == shapes[k]
    assert fx['weight_checksum'].shape == (4,)


def test_v_fullsize_golden_weight_checksums_match_the_seeded_networks(golden_dir):
    torch.set_num_threads(min(16, os.cpu_count() or 8))
    try:
        fx = np.load(os.path.join(golden_dir, 'fullsize_sd21v_k2_512.npz'))
        cks = np.array(fixtures.checksum(fixtures.make_unet_cached('sd21-base')) + fixtures.checksum(fixtures.make_unet_cached('sd21-base', seed=77)))
        assert np.all(np.abs(cks - fx['weight_checksum']) <= 1e-9 * np.abs(fx['weight_checksum']))
    finally:
        torch.set_num_threads(min(8, os.cpu_count() or 8))
