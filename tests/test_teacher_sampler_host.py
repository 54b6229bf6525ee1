"""Sampling the teacher itself (guided multi-step DDIM), host side: the DDIM schedule against an fp64 restatement of the published
index arithmetic (Song et al. 2021; diffusers' DDIMScheduler.set_timesteps / step with 'leading' spacing), its refusals, and the new
option values of the two command lines (`--network teacher`, `--network_pkl teacher`)."""
import inspect
import os

import pytest
import torch

SD = dict(steps_offset=1, set_alpha_to_one=False, timestep_spacing='leading')


def _restated(T, N, offset, alpha_to_one):
    """fp64 restatement: betas scaled_linear 0.00085 .. 0.012, abar = cumprod(1 - beta); t_i = (N-1-i)*(T//N) + offset; prev = t - T//N."""
    betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, T, dtype=torch.float64) ** 2
    abar = torch.cumprod(1 - betas, 0)
    ratio = T // N
    t = [(N - 1 - i) * ratio + offset for i in range(N)]
    prev = [x - ratio for x in t]
    return abar, t, prev


@pytest.mark.parametrize('N', [50, 4, 1])
@pytest.mark.parametrize('alpha_to_one', [False, True])
def test_ddim_schedule_matches_the_restated_formulas(N, alpha_to_one):
    from sid_lsg_amd.scheduler import DDPMScheduler, ddim_schedule
    sched = DDPMScheduler()
    cfg = dict(SD, set_alpha_to_one=alpha_to_one)
    ts, s0, s1, s0p, s1p = ddim_schedule(sched, cfg, N)
    abar64, t, prev = _restated(1000, N, 1, alpha_to_one)
    assert ts.dtype == torch.long and ts.tolist() == t
    if N == 50:
        assert t == list(range(981, 0, -20)) and t[0] == 981 and t[-1] == 1
    assert all(v.dtype == torch.float32 and v.shape == (N,) for v in (s0, s1, s0p, s1p))
    # exactly the scheduler's own fp32 table gathered at the restated indices
    abar = sched.alphas_cumprod
    a_t = abar[torch.tensor(t)]
    final = torch.tensor(1.0) if alpha_to_one else abar[0]
    a_p = torch.stack([abar[p] if p >= 0 else final for p in prev])
    assert torch.equal(s0, a_t ** 0.5) and torch.equal(s1, (1 - a_t) ** 0.5)
    assert torch.equal(s0p, a_p ** 0.5) and torch.equal(s1p, (1 - a_p) ** 0.5)
    assert torch.equal(s0, sched.coefficients(ts)[0]) and torch.equal(s1, sched.coefficients(ts)[1])
    # and the fp64 restatement, to the rounding of the fp32 table: every factor 1 - beta_j is rounded once (beta_j's own error is
    # below 0.012 of that) and every partial product once, so abar_t carries at most 2 (t + 1) half-ulps, plus 2 for the final
    # subtraction and square root: n * 2^-24 relative on abar; sqrt halves it; on sqrt(1 - abar) the absolute error of abar is
    # divided by 2 sqrt(1 - abar).  One more half-ulp for the rounding of the result itself.
    u = 2.0 ** -24
    for got, idx, one_minus in ((s0, t, False), (s1, t, True), (s0p, prev, False), (s1p, prev, True)):
        for g, i in zip(got.tolist(), idx):
            a = float(abar64[i]) if i >= 0 else (1.0 if alpha_to_one else float(abar64[0]))
            n = 2 * (max(i, 0) + 1) + 2
            want = (1 - a) ** 0.5 if one_minus else a ** 0.5
            err = (n * u * a) / (2 * want) + u * want if want > 0 else 0.0
            assert abs(g - want) <= err, (i, g, want, err)
    # the last step lands on the final alpha
    if alpha_to_one:
        assert float(s0p[-1]) == 1.0 and float(s1p[-1]) == 0.0
    else:
        assert float(s0p[-1]) == float(abar[0] ** 0.5)
    assert prev[-1] < 0


def test_ddim_schedule_defaults_are_diffusers_defaults():
    """No config: steps_offset 0, set_alpha_to_one true."""
    from sid_lsg_amd.scheduler import DDPMScheduler, ddim_schedule
    ts, s0, s1, s0p, s1p = ddim_schedule(DDPMScheduler(), None, 4)
    assert ts.tolist() == [750, 500, 250, 0] and float(s0p[-1]) == 1.0 and float(s1p[-1]) == 0.0


@pytest.mark.parametrize('cfg,N,key', [(dict(SD, timestep_spacing='trailing'), 50, 'timestep_spacing'), (SD, 0, 'num_inference_steps'),
                                       (SD, 1001, 'num_inference_steps'), (dict(SD, steps_offset=1), 1000, 'steps_offset'),
                                       (dict(SD, steps_offset=600), 2, 'steps_offset')])
def test_ddim_schedule_refusals_name_the_key(cfg, N, key):
    from sid_lsg_amd.scheduler import DDPMScheduler, ddim_schedule
    with pytest.raises(ValueError, match=key):
        ddim_schedule(DDPMScheduler(), cfg, N)


def test_sampling_config_comes_with_the_resolved_scheduler(tmp_path):
    """resolve_scheduler: the sampling keys of <dir>/scheduler/scheduler_config.json (diffusers' defaults for absent ones), the SD
    values for seeded random networks; the scheduler itself is what it was."""
    import json

    from sid_lsg_amd.scheduler import ddim_schedule
    from sid_lsg_amd.sd_util import resolve_scheduler
    for spec, pt in (('random:tiny', 'epsilon'), ('random:tiny:v', 'v_prediction')):
        s = resolve_scheduler(spec)
        assert s.sampling_config == SD and s.config.prediction_type == pt
    d = tmp_path / 'model' / 'scheduler'
    d.mkdir(parents=True)
    (d / 'scheduler_config.json').write_text(json.dumps(dict(beta_schedule='scaled_linear', beta_start=0.00085, beta_end=0.012,
                                                             num_train_timesteps=1000, steps_offset=1, set_alpha_to_one=False,
                                                             prediction_type='v_prediction', clip_sample=False)))
    s = resolve_scheduler(str(tmp_path / 'model'))
    assert s.sampling_config == dict(steps_offset=1, set_alpha_to_one=False) and s.config.prediction_type == 'v_prediction'
    assert ddim_schedule(s, s.sampling_config, 50)[0][0] == 981
    (d / 'scheduler_config.json').write_text(json.dumps(dict(beta_schedule='scaled_linear', beta_start=0.00085, beta_end=0.012)))
    s = resolve_scheduler(str(tmp_path / 'model'))
    assert s.sampling_config == {}
    # what teacher_sample hands to ddim_schedule: an empty dict is a file without the keys, i.e. diffusers' defaults (offset 0, final
    # alpha 1), not a missing config; a partial file gets the defaults for the absent keys; an explicit argument wins
    from sid_lsg_amd.sd_util import sampling_config_of
    assert sampling_config_of(s) == {}
    ts, _, _, s0p, s1p = ddim_schedule(s, sampling_config_of(s), 4)
    assert ts.tolist() == [750, 500, 250, 0] and float(s0p[-1]) == 1.0 and float(s1p[-1]) == 0.0
    (d / 'scheduler_config.json').write_text(json.dumps(dict(beta_schedule='scaled_linear', beta_start=0.00085, beta_end=0.012, steps_offset=1)))
    s = resolve_scheduler(str(tmp_path / 'model'))
    assert sampling_config_of(s) == dict(steps_offset=1)
    ts, _, _, s0p, _ = ddim_schedule(s, sampling_config_of(s), 4)
    assert ts.tolist() == [751, 501, 251, 1] and float(s0p[-1]) == 1.0
    assert sampling_config_of(s, SD) is SD
    from sid_lsg_amd.scheduler import DDPMScheduler
    assert sampling_config_of(DDPMScheduler()) == SD          # a scheduler built by hand: the SD values


def test_teacher_sample_signature():
    from sid_lsg_amd.sd_util import teacher_sample
    p = inspect.signature(teacher_sample).parameters
    assert list(p) == ['unet', 'latents', 'contexts', 'noise_scheduler', 'text_encoder', 'tokenizer', 'resolution', 'guidance_scale',
                       'num_inference_steps', 'return_images', 'vae', 'schedule_config']
    assert p['guidance_scale'].default == 7.5 and p['num_inference_steps'].default == 50 and p['return_images'].default is False
    with pytest.raises(TypeError, match='HipUNet2DCondition'):
        teacher_sample(torch.nn.Linear(1, 1), torch.zeros(1, 4, 8, 8), ['x'], None, None, None, 64)


# ---- command lines ----------------------------------------------------------------------------------------------------------------
def _options(tmp_path, **over):
    import sid_train
    o = dict(outdir='x', data=None, data_stat=None, data_prompt_text=str(tmp_path), duration=0.01, batch=8, batch_gpu=2, ema=0.05,
             xflip=0.0, bench=True, cache=True, workers=1, desc=None, nosubdir=False, tick=2, snap=50, dump=100, seed=3, transfer=None,
             resume=None, dry_run=True, metrics=None, sd_model='random:tiny', resolution=512, init_timestep=625, fp16=False, ls=1, lsg=1,
             alpha=1, tmax=980, tmin=20, lr=1e-6, glr=2e-6, train_mode=True, network_pkl=None, cfg_train_fake=1.5, cfg_eval_fake=1.5,
             cfg_eval_real=1.5, metric_pt_path=None, metric_clip_path=None, metric_open_clip_path=None, enable_xformers=True,
             gradient_checkpointing=False, optimizer='adam', num_steps=1, fake_score_use_lora=False)
    o.update(over)
    return sid_train.EasyDict(o)


def _metric_files(tmp_path):
    det, stat = tmp_path / 'det.pt', tmp_path / 'stat.npz'
    det.write_bytes(b'x')
    stat.write_bytes(b'x')
    (tmp_path / 'aesthetics_6_plus.txt').write_text('a red cube\na blue sphere\n')
    return dict(metrics=['fid_test'], metric_pt_path=str(det), data_stat=str(stat))


def test_sid_train_accepts_the_teacher_sentinel(tmp_path):
    import click
    import sid_train
    from sid_lsg_amd.training_loop import training_loop
    m = _metric_files(tmp_path)
    ev = dict(m, train_mode=False, network_pkl='teacher')
    c = sid_train.build_config(_options(tmp_path, **ev))
    assert c.network_pkl == 'teacher' and c.train_mode is False and c.teacher_steps == 50 and c.teacher_cfg == 7.5
    inspect.signature(training_loop).bind(**c)                        # every key is a keyword of the loop
    c = sid_train.build_config(_options(tmp_path, teacher_steps=3, teacher_cfg=2.0, **ev))
    assert c.teacher_steps == 3 and c.teacher_cfg == 2.0
    assert sid_train.build_config(_options(tmp_path, teacher_steps=1000, **ev)).teacher_steps == 1000
    for steps in (0, -1, 1001):
        with pytest.raises(click.ClickException, match='--teacher_steps'):
            sid_train.build_config(_options(tmp_path, teacher_steps=steps, **ev))
    # the teacher's options with a real snapshot, or while training, are refused
    snap = tmp_path / 'network-snapshot-1.000000-000001.pkl'
    snap.write_bytes(b'x')
    for over in (dict(m, train_mode=False, network_pkl=str(snap), teacher_steps=3), dict(m, train_mode=False, network_pkl=str(snap), teacher_cfg=2.0),
                 dict(teacher_steps=3), dict(network_pkl='teacher', teacher_cfg=2.0)):
        with pytest.raises(click.ClickException, match='teacher'):
            sid_train.build_config(_options(tmp_path, **over))
    # a snapshot that does not exist is still refused; a real one still passes, with no teacher key in the config
    with pytest.raises(click.ClickException, match='--network_pkl'):
        sid_train.build_config(_options(tmp_path, **dict(m, train_mode=False, network_pkl=str(tmp_path / 'missing.pkl'))))
    c = sid_train.build_config(_options(tmp_path, **dict(m, train_mode=False, network_pkl=str(snap))))
    assert 'teacher_steps' not in c and 'teacher_cfg' not in c


def test_existing_invocations_build_the_same_config(tmp_path):
    """A distillation run: the config has exactly the keys it had, whether the options object knows the new options or not."""
    import sid_train
    (tmp_path / 'aesthetics_6_plus.txt').write_text('a red cube\n')
    a = sid_train.build_config(_options(tmp_path))
    b = sid_train.build_config(_options(tmp_path, teacher_steps=None, teacher_cfg=None))
    assert dict(a) == dict(b) and 'teacher_steps' not in a and 'teacher_cfg' not in a
    assert sorted(a) == sorted([
        'alpha', 'batch_gpu', 'batch_size', 'cfg_eval_fake', 'cfg_eval_real', 'cfg_train_fake', 'cudnn_benchmark', 'data_loader_kwargs',
        'dataset_prompt_text_kwargs', 'deterministic', 'ema_halflife_kimg', 'enable_xformers', 'fake_score_optimizer_kwargs',
        'fake_score_use_lora', 'g_optimizer_kwargs', 'gradient_checkpointing', 'init_timestep', 'kimg_per_tick', 'loss_kwargs',
        'loss_scaling', 'loss_scaling_G', 'metric_clip_path', 'metric_open_clip_path', 'metric_pt_path', 'metric_real_stats', 'metrics',
        'network_kwargs', 'network_pkl', 'num_steps', 'pretrained_model_name_or_path', 'pretrained_vae_model_name_or_path', 'resolution',
        'snapshot_ticks', 'state_dump_ticks', 'tmax', 'tmin', 'total_kimg', 'train_mode'])
    opts = {f[0]: kw for f, kw in sid_train.OPTIONS}
    assert opts['--teacher_steps']['default'] is None and opts['--teacher_cfg']['default'] is None


def test_sid_train_dry_run_with_the_teacher(tmp_path):
    from click.testing import CliRunner
    import sid_train
    m = _metric_files(tmp_path)
    base = ['--outdir', str(tmp_path / 'runs'), '--data_prompt_text', str(tmp_path), '--sd_model', 'random:tiny', '--seed', '1', '--train_mode', '0',
            '--metrics', 'fid_test', '--metric_pt_path', m['metric_pt_path'], '--data_stat', m['data_stat'], '--dry-run']
    ok = CliRunner().invoke(sid_train.main, base + ['--network_pkl', 'teacher', '--teacher_steps', '3', '--teacher_cfg', '2'])
    assert ok.exit_code == 0, ok.output
    assert '"teacher_steps": 3' in ok.output and '"teacher_cfg": 2.0' in ok.output
    bad = CliRunner().invoke(sid_train.main, base + ['--network_pkl', 'teacher', '--teacher_steps', '0'])
    assert bad.exit_code != 0 and '--teacher_steps' in bad.output


def test_generate_onestep_teacher_options(tmp_path):
    import click
    from click.testing import CliRunner
    import generate_onestep as g
    assert g.teacher_options('teacher', None, None) == (50, 7.5)
    assert g.teacher_options('teacher', 3, 2.0) == (3, 2.0)
    assert g.teacher_options('snap.pkl', None, None) is None
    for steps, scale in ((3, None), (None, 2.0)):
        with pytest.raises(click.UsageError, match='--network teacher'):
            g.teacher_options('snap.pkl', steps, scale)
    # refused by the command line before anything is loaded
    snap = tmp_path / 'network-snapshot.pkl'
    snap.write_bytes(b'x')
    common = ['--outdir', str(tmp_path / 'out'), '--seeds', '0-1', '--repo_id', 'random:tiny']
    res = CliRunner().invoke(g.main, ['--network', str(snap), '--teacher_steps', '3'] + common)
    assert res.exit_code != 0 and '--teacher_steps' in res.output and not os.path.exists(tmp_path / 'out')
    res = CliRunner().invoke(g.main, ['--network', str(snap), '--guidance_scale', '2'] + common)
    assert res.exit_code != 0 and '--guidance_scale' in res.output
    res = CliRunner().invoke(g.main, ['--network', 'teacher', '--teacher_steps', '0'] + common)
    assert res.exit_code != 0 and 'teacher_steps' in res.output
    names = [p.name for p in g.main.params]
    assert 'teacher_steps' in names and 'guidance_scale' in names
    by = {p.name: p for p in g.main.params}
    assert by['teacher_steps'].default is None and by['guidance_scale'].default is None and by['num_steps_eval'].default == 1


def test_ddim_step_is_declared_and_bound():
    """Both entry points are in the header with the documented argument list, and ops.ddim_step refuses tensors that want gradients
    before it touches the device."""
    import ctypes

    from sid_lsg_amd import ops
    from sid_lsg_amd._lib import parse_header
    protos = parse_header()
    want = [ctypes.c_void_p] * 9 + [ctypes.c_int] * 6 + [ctypes.c_float, ctypes.c_int, ctypes.c_void_p]
    assert protos['sidlsg_ddim_step'] == want and protos['sidlsg_ddim_step_f32'] == want
    x = torch.zeros(1, 4, 2, 2, requires_grad=True)
    e = torch.zeros(1, 4, 8)
    s = torch.ones(1)
    with pytest.raises(RuntimeError, match='forward only'):
        ops.ddim_step(e, x, s, s, s, s, 1.0)
