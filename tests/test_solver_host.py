"""The teacher's solver family (DPM-Solver++ 2M, DDIM with any eta, 'leading' / 'trailing' / 'linspace' spacing, guidance rescale), host
side: scheduler.solver_schedule against the quoted timestep sets and an fp64 restatement of the published update rules written here,
its identities and refusals, the order of the 2M update against an analytic denoiser, and the new options of the two command lines."""
import ctypes
import inspect
import math
import os

import numpy as np
import pytest
import torch

SD = dict(steps_offset=1, set_alpha_to_one=False, timestep_spacing='leading')
T = 1000


def _sched():
    from sid_lsg_amd.scheduler import DDPMScheduler
    return DDPMScheduler()


def _abar64(sched):
    """The scheduler's own fp32 table, as fp64 values: what the schedule is specified to start from."""
    return [float(v) for v in sched.alphas_cumprod.tolist()]


# ---- timestep sets -------------------------------------------------------------------------------------------------------------------
def test_the_quoted_timestep_sets():
    from sid_lsg_amd.scheduler import solver_schedule
    s = _sched()
    ts = lambda *a, **k: solver_schedule(s, *a, **k)[0].tolist()  # noqa: E731
    assert ts(SD, 4, 'dpmpp2m', 'leading') == [801, 601, 401, 201]
    assert ts(dict(SD, steps_offset=0), 4, 'dpmpp2m', 'leading') == [800, 600, 400, 200]
    assert ts(SD, 4, 'dpmpp2m', 'trailing') == [999, 749, 499, 249]
    assert ts(SD, 4, 'dpmpp2m', 'linspace') == [999, 749, 500, 250]
    assert ts(SD, 3, 'ddim', 'trailing') == [999, 666, 332]
    assert ts(SD, 1, 'dpmpp2m', 'trailing') == [999] and ts(SD, 1, 'ddim', 'trailing') == [999]
    assert ts(SD, 4, 'ddim', 'leading') == [751, 501, 251, 1] and ts(dict(SD, steps_offset=0), 4, 'ddim', 'leading') == [750, 500, 250, 0]
    # spacing None takes the model's timestep_spacing, 'leading' when it has none; trailing ignores steps_offset
    assert ts(dict(SD, timestep_spacing='trailing'), 4) == [999, 749, 499, 249] and ts({}, 4) == [800, 600, 400, 200]
    assert ts(dict(SD, steps_offset=0), 4, 'dpmpp2m', 'trailing') == [999, 749, 499, 249]
    t, s0, s1, coef = solver_schedule(s, SD, 4)
    assert t.dtype == torch.long and s0.dtype == s1.dtype == coef.dtype == torch.float32
    assert s0.shape == s1.shape == (4,) and coef.shape == (4, 4)
    # alpha / sigma at t_i: fp64 square roots of abar and 1 - abar rounded once; the scheduler's own sigma table forms 1 - abar in fp32
    # first, which may differ in the last place
    assert torch.equal(s0, s.coefficients(t)[0])
    assert bool(((s1 - s.coefficients(t)[1]).abs() <= torch.from_numpy(np.spacing(s1.numpy()))).all())
    assert torch.equal(s1, (1 - s.alphas_cumprod[t].double()).sqrt().float())


def test_ddim_trailing_targets():
    """'ddim' 'trailing' at N = 3: the targets are t_i - T//N = [666, 333, final], read off the coefficients: with eta = 0,
    c_x = sigma_target / sigma_t."""
    from sid_lsg_amd.scheduler import solver_schedule
    s = _sched()
    abar = _abar64(s)
    for one in (False, True):
        t, s0, s1, coef = solver_schedule(s, dict(SD, set_alpha_to_one=one), 3, 'ddim', 'trailing')
        targets = [abar[666], abar[333], 1.0 if one else abar[0]]
        for i in range(3):
            want = math.sqrt(1 - targets[i]) / math.sqrt(1 - abar[t[i]])
            assert abs(float(coef[i, 0]) - want) <= 2 * float(np.spacing(np.float32(want)))
    assert coef[2].tolist() == [0.0, 1.0, 0.0, 0.0]


@pytest.mark.parametrize('kw,name', [
    (dict(solver='ddim', spacing='linspace'), 'spacing'), (dict(solver='dpmpp2m', eta=0.5), 'eta'), (dict(solver='ddim', eta=-1.0), 'eta'),
    (dict(num_inference_steps=0), 'num_inference_steps'), (dict(num_inference_steps=-2), 'num_inference_steps'),
    (dict(num_inference_steps=T + 1), 'num_inference_steps'),
    (dict(num_inference_steps=T, solver='dpmpp2m', spacing='leading'), 'num_inference_steps'),      # T // (N + 1) = 0: all equal
    (dict(num_inference_steps=T, solver='dpmpp2m', spacing='linspace'), 'num_inference_steps'),     # 1001 points on 1000 integers
    (dict(config_dict=dict(SD, steps_offset=300)), 'steps_offset'), (dict(config_dict=dict(SD, steps_offset=-1)), 'steps_offset'),
    (dict(solver='heun'), 'solver'), (dict(spacing='karras'), 'spacing'), (dict(config_dict=dict(SD, timestep_spacing='karras')), 'spacing'),
])
def test_refusals_name_the_argument(kw, name):
    from sid_lsg_amd.scheduler import solver_schedule
    kw = dict(dict(config_dict=SD, num_inference_steps=4), **kw)
    with pytest.raises(ValueError, match=rf'^{name}='):
        solver_schedule(_sched(), **kw)


def test_every_admitted_count_gives_strictly_decreasing_timesteps_in_range():
    from sid_lsg_amd.scheduler import solver_schedule
    s = _sched()
    for solver, spacing in (('ddim', 'leading'), ('ddim', 'trailing'), ('dpmpp2m', 'leading'), ('dpmpp2m', 'trailing'), ('dpmpp2m', 'linspace')):
        for N in (1, 2, 3, 7, 50, 333, 499, 500):
            t = solver_schedule(s, SD, N, solver, spacing)[0].tolist()
            assert len(t) == N and all(a > b for a, b in zip(t, t[1:])) and 0 <= t[-1] and t[0] < T, (solver, spacing, N)


# ---- the coefficients against an fp64 restatement written here --------------------------------------------------------------------------
def _timesteps(solver, spacing, N, offset):
    if spacing == 'trailing':
        return [int(np.round(T - i * T / N)) - 1 for i in range(N)]
    if spacing == 'linspace':
        return [int(v) for v in np.round(np.linspace(0, T - 1, N + 1))[::-1][:-1]]
    if solver == 'ddim':
        return [(N - 1 - i) * (T // N) + offset for i in range(N)]
    return [(N - i) * (T // (N + 1)) + offset for i in range(N)]


def _lam(a):
    return math.log(math.sqrt(a) / math.sqrt(1 - a))


def _restated(abar, solver, spacing, N, offset=1, alpha_to_one=False, eta=0.0):
    """-> (timesteps, rows) from the lambda / alpha / sigma formulas of the update rules, in python floats."""
    t = _timesteps(solver, spacing, N, offset)
    if solver == 'ddim':
        target = [abar[p] if p >= 0 else (1.0 if alpha_to_one else abar[0]) for p in (x - T // N for x in t)]
    else:
        target = [abar[x] for x in t[1:]] + [1.0]
    rows = []
    for i in range(N):
        a_s, a_t = abar[t[i]], target[i]
        if a_t == 1.0:
            rows.append((0.0, 1.0, 0.0, 0.0))
            continue
        al_s, sg_s, al_t, sg_t = math.sqrt(a_s), math.sqrt(1 - a_s), math.sqrt(a_t), math.sqrt(1 - a_t)
        if solver == 'ddim':
            sg_eta = eta * math.sqrt((1 - a_t) / (1 - a_s)) * math.sqrt(1 - a_s / a_t)
            cx = math.sqrt(sg_t * sg_t - sg_eta * sg_eta) / sg_s
            rows.append((cx, al_t - cx * al_s, 0.0, sg_eta))
            continue
        h = _lam(a_t) - _lam(a_s)
        A = al_t * (1 - math.exp(-h))
        if i == 0:
            rows.append((sg_t / sg_s, A, 0.0, 0.0))
        else:
            r0 = (_lam(a_s) - _lam(abar[t[i - 1]])) / h
            rows.append((sg_t / sg_s, A * (1 + 0.5 / r0), -A * 0.5 / r0, 0.0))
    return t, rows


def _assert_rows(coef, rows, what):
    assert coef.shape == (len(rows), 4)
    for i, row in enumerate(rows):
        for j, want in enumerate(row):
            got = float(coef[i, j])
            ulp = float(np.spacing(np.float32(abs(want)))) if want != 0 else 0.0
            assert abs(got - want) <= 2 * ulp, (what, i, j, got, want)


@pytest.mark.parametrize('eta', [0.0, 0.5, 1.0])
@pytest.mark.parametrize('spacing', ['leading', 'trailing'])
@pytest.mark.parametrize('N', [1, 3, 50])
def test_ddim_coefficients_match_the_restatement(N, spacing, eta):
    from sid_lsg_amd.scheduler import solver_schedule
    s = _sched()
    for offset, one in ((1, False), (0, True)):
        cfg = dict(steps_offset=offset, set_alpha_to_one=one)
        t, s0, s1, coef = solver_schedule(s, cfg, N, 'ddim', spacing, eta)
        want_t, rows = _restated(_abar64(s), 'ddim', spacing, N, offset, one, eta)
        assert t.tolist() == want_t
        _assert_rows(coef, rows, ('ddim', N, spacing, eta, offset))
        assert bool((coef[:, 2] == 0).all())
        assert bool((coef[:, 3] == 0).all()) == (eta == 0 or (N == 1 and one))
        if one:
            assert coef[-1].tolist() == [0.0, 1.0, 0.0, 0.0]         # onto abar = 1: sigma_eta = 0 and x_t is the x0 prediction


@pytest.mark.parametrize('spacing', ['leading', 'trailing', 'linspace'])
@pytest.mark.parametrize('N', [1, 2, 4, 20])
def test_dpmpp2m_coefficients_match_the_restatement(N, spacing):
    from sid_lsg_amd.scheduler import solver_schedule
    s = _sched()
    for offset in (0, 1):
        t, s0, s1, coef = solver_schedule(s, dict(SD, steps_offset=offset), N, 'dpmpp2m', spacing)
        want_t, rows = _restated(_abar64(s), 'dpmpp2m', spacing, N, offset)
        assert t.tolist() == want_t
        _assert_rows(coef, rows, ('dpmpp2m', N, spacing, offset))
        assert coef[-1].tolist() == [0.0, 1.0, 0.0, 0.0] and bool(torch.isfinite(coef).all())
        assert bool((coef[:, 3] == 0).all()) and float(coef[0, 2]) == 0.0
        if N > 2:
            assert bool((coef[1:-1, 2] < 0).all()) and bool((coef[1:-1, 1] > 0).all())


# ---- identities ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', [1, 4, 50])
@pytest.mark.parametrize('one', [False, True])
def test_ddim_eta_zero_leading_is_ddim_schedule(N, one):
    """x_prev = s0p*x0 + s1p*eps_hat with eps_hat = (x - s0*x0)/s1 is c_x = s1p/s1, c_cur = s0p - s0*s1p/s1."""
    from sid_lsg_amd.scheduler import ddim_schedule, solver_schedule
    s = _sched()
    cfg = dict(SD, set_alpha_to_one=one)
    ts, s0, s1, s0p, s1p = ddim_schedule(s, cfg, N)
    t, a0, a1, coef = solver_schedule(s, cfg, N, 'ddim', 'leading', 0.0)
    assert torch.equal(t, ts) and torch.equal(a0, s0) and bool(((a1 - s1).abs() <= torch.from_numpy(np.spacing(s1.numpy()))).all())
    s0, s1, s0p, s1p = (v.double() for v in (s0, s1, s0p, s1p))
    cx = s1p / s1
    # ddim_schedule's values are fp32 roundings of the square roots (half an ulp each), the coefficients are formed from the
    # unrounded ones: c_x carries two of them and its own rounding, c_cur = s0p - s0*c_x up to four on terms of size <= 1
    u = 2.0 ** -24
    assert bool(((coef[:, 0].double() - cx).abs() <= 3 * u * cx + 1e-12).all())
    assert bool(((coef[:, 1].double() - (s0p - s0 * cx)).abs() <= 5 * u).all())


def test_dpmpp2m_one_step_is_the_x0_prediction():
    from sid_lsg_amd.scheduler import solver_schedule
    for spacing in ('leading', 'trailing', 'linspace'):
        assert solver_schedule(_sched(), SD, 1, 'dpmpp2m', spacing)[3].tolist() == [[0.0, 1.0, 0.0, 0.0]]


def test_first_order_dpmpp2m_row_is_the_ddim_row():
    """alpha_t (1 - exp(-h)) = alpha_t - alpha_s sigma_t / sigma_s: the same (s, t) pair gives the same row.  'trailing' N = 4 has the
    pair (999, 749) as the first step of both solvers (749 = 999 - T//4)."""
    from sid_lsg_amd.scheduler import solver_schedule
    s = _sched()
    a = solver_schedule(s, SD, 4, 'dpmpp2m', 'trailing')
    b = solver_schedule(s, SD, 4, 'ddim', 'trailing', 0.0)
    assert a[0].tolist()[:2] == [999, 749] and b[0].tolist()[:2] == [999, 749]
    for j in range(4):
        want = float(b[3][0, j])
        assert abs(float(a[3][0, j]) - want) <= 2 * float(np.spacing(np.float32(abs(want)))), j


# ---- the order of the 2M update, with an analytic denoiser ----------------------------------------------------------------------------
@pytest.mark.parametrize('spacing', ['leading', 'trailing'])
@pytest.mark.parametrize('N', [10, 20, 40])
@pytest.mark.parametrize('std', [0.5, 1.5])
def test_dpmpp2m_beats_its_first_order_half_on_gaussian_data(std, N, spacing):
    """Data N(0, std^2): the ideal denoiser is x0*(x, t) = sqrt(abar) std^2 x / (abar std^2 + 1 - abar) and the probability-flow state
    at t is x_{t0} sqrt(abar_t std^2 + 1 - abar_t) / sqrt(abar_{t0} std^2 + 1 - abar_{t0}).  The fp64 tables run up to t_{N-1}; the 2M
    error is at most a quarter of the error of the same schedule with c_prev = 0 and c_cur = A (a wrong sign or r0 gives more than 1).
    The full chain returns exactly the last x0 prediction."""
    from sid_lsg_amd.scheduler import solver_tables
    s = _sched()
    abar = _abar64(s)
    t, al, sg, coef = solver_tables(s, SD, N, 'dpmpp2m', spacing)
    assert coef.dtype == np.float64
    v2 = std * std
    x0_of = lambda x, a: math.sqrt(a) * v2 * x / (a * v2 + 1 - a)  # noqa: E731
    exact = lambda a: math.sqrt(a * v2 + 1 - a) / math.sqrt(abar[t[0]] * v2 + 1 - abar[t[0]])  # noqa: E731
    x2 = x1 = 1.0
    prev = 0.0
    for i in range(N - 1):
        a_s, a_t = abar[t[i]], abar[t[i + 1]]
        d = x0_of(x2, a_s)
        x2 = coef[i, 0] * x2 + coef[i, 1] * d + coef[i, 2] * prev
        prev = d
        A = math.sqrt(a_t) * (1 - math.exp(_lam(a_s) - _lam(a_t)))
        x1 = math.sqrt(1 - a_t) / math.sqrt(1 - a_s) * x1 + A * x0_of(x1, a_s)
    want = exact(abar[t[N - 1]])
    e2, e1 = abs(x2 - want), abs(x1 - want)
    print(f'std {std} N {N} {spacing}: 2M error {e2:.3e}, first order {e1:.3e}, ratio {e2 / e1:.3f}')
    assert e1 > 0 and e2 <= 0.25 * e1, (e2, e1)
    last = x0_of(x2, abar[t[N - 1]])
    assert coef[N - 1, 0] * x2 + coef[N - 1, 1] * last + coef[N - 1, 2] * prev == last


# ---- command lines -----------------------------------------------------------------------------------------------------------------------
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


NEW_KEYS = ('teacher_sampler', 'teacher_spacing', 'teacher_eta', 'teacher_rescale')


def test_sid_train_solver_options(tmp_path):
    import click
    import sid_train
    from sid_lsg_amd.training_loop import training_loop
    m = _metric_files(tmp_path)
    ev = dict(m, train_mode=False, network_pkl='teacher')
    opts = {f[0]: kw for f, kw in sid_train.OPTIONS}
    assert all(opts[f'--{k}']['default'] is None for k in NEW_KEYS)
    # absent unless given: the teacher's config, and a distillation run's, have the keys they had
    c = sid_train.build_config(_options(tmp_path, **ev))
    assert not any(k in c for k in NEW_KEYS)
    assert dict(c) == dict(sid_train.build_config(_options(tmp_path, **dict(ev, **{k: None for k in NEW_KEYS}))))
    assert not any(k in sid_train.build_config(_options(tmp_path)) for k in NEW_KEYS)
    c = sid_train.build_config(_options(tmp_path, teacher_sampler='dpmpp2m', teacher_spacing='trailing', teacher_rescale=0.7, teacher_steps=20, **ev))
    assert c.teacher_sampler == 'dpmpp2m' and c.teacher_spacing == 'trailing' and c.teacher_rescale == 0.7 and 'teacher_eta' not in c
    inspect.signature(training_loop).bind(**c)                        # every key is a keyword of the loop
    c = sid_train.build_config(_options(tmp_path, teacher_eta=1, **ev))
    assert c.teacher_eta == 1.0 and isinstance(c.teacher_eta, float) and 'teacher_sampler' not in c
    inspect.signature(training_loop).bind(**c)
    # refused with a snapshot or while training
    snap = tmp_path / 'network-snapshot-1.000000-000001.pkl'
    snap.write_bytes(b'x')
    for k, v in (('teacher_sampler', 'dpmpp2m'), ('teacher_spacing', 'trailing'), ('teacher_eta', 0.5), ('teacher_rescale', 0.7)):
        for over in (dict(m, train_mode=False, network_pkl=str(snap)), dict(), dict(network_pkl='teacher')):
            with pytest.raises(click.ClickException, match=f'--{k}'):
                sid_train.build_config(_options(tmp_path, **dict(over, **{k: v})))
    # combinations the schedule refuses are refused here, by name
    with pytest.raises(click.ClickException, match='--teacher_eta'):
        sid_train.build_config(_options(tmp_path, teacher_sampler='dpmpp2m', teacher_eta=0.5, **ev))
    with pytest.raises(click.ClickException, match='--teacher_spacing'):
        sid_train.build_config(_options(tmp_path, teacher_spacing='linspace', **ev))


def test_sid_train_dry_run_with_the_solver_options(tmp_path):
    from click.testing import CliRunner
    import sid_train
    m = _metric_files(tmp_path)
    base = ['--outdir', str(tmp_path / 'runs'), '--data_prompt_text', str(tmp_path), '--sd_model', 'random:tiny', '--seed', '1', '--train_mode', '0',
            '--metrics', 'fid_test', '--metric_pt_path', m['metric_pt_path'], '--data_stat', m['data_stat'], '--dry-run', '--network_pkl', 'teacher']
    ok = CliRunner().invoke(sid_train.main, base + ['--teacher_sampler', 'dpmpp2m', '--teacher_steps', '4', '--teacher_rescale', '0.7'])
    assert ok.exit_code == 0, ok.output
    assert '"teacher_sampler": "dpmpp2m"' in ok.output and '"teacher_rescale": 0.7' in ok.output and 'teacher_eta' not in ok.output
    plain = CliRunner().invoke(sid_train.main, base)
    assert plain.exit_code == 0 and not any(k in plain.output for k in NEW_KEYS)
    bad = CliRunner().invoke(sid_train.main, base + ['--teacher_sampler', 'heun'])
    assert bad.exit_code != 0 and '--teacher_sampler' in bad.output


def test_report_names():
    from sid_lsg_amd.training_loop import evaluate_teacher, teacher_report_name, teacher_solver_kwargs
    assert teacher_report_name(50, 7.5) == 'teacher-ddim50-cfg7.5'                      # the name the default has always had
    assert teacher_report_name(3, 2.0) == 'teacher-ddim3-cfg2'
    assert teacher_report_name(20, 7.5, 'dpmpp2m') == 'teacher-dpmpp2m20-cfg7.5'
    assert teacher_report_name(20, 7.5, 'dpmpp2m', 'trailing', None, 0.7) == 'teacher-dpmpp2m20-trailing-rs0.7-cfg7.5'
    assert teacher_report_name(50, 7.5, 'ddim', None, 1.0) == 'teacher-ddim50-eta1-cfg7.5'
    assert teacher_report_name(1, 1, None, 'trailing', 0.5, 0.25) == 'teacher-ddim1-trailing-eta0.5-rs0.25-cfg1'
    assert teacher_solver_kwargs() is None
    assert teacher_solver_kwargs(None, 'trailing') == dict(solver='ddim', spacing='trailing', eta=0.0, guidance_rescale=0.0)
    assert teacher_solver_kwargs('dpmpp2m', None, None, 0.7) == dict(solver='dpmpp2m', spacing=None, eta=0.0, guidance_rescale=0.7)
    p = inspect.signature(evaluate_teacher).parameters
    assert all(p[k].default is None for k in NEW_KEYS)


def test_generate_onestep_solver_options(tmp_path):
    import click
    from click.testing import CliRunner
    import generate_onestep as g
    assert g.teacher_solver_options('teacher') is None and g.teacher_solver_options('snap.pkl') is None
    assert g.teacher_options('teacher', None, None) == (50, 7.5)                          # the existing helper is as it was
    assert list(inspect.signature(g.teacher_options).parameters) == ['network_pkl', 'teacher_steps', 'guidance_scale']
    assert g.teacher_solver_options('teacher', 'dpmpp2m') == dict(solver='dpmpp2m', spacing=None, eta=0.0, guidance_rescale=0.0, negative_prompt=None)
    assert g.teacher_solver_options('teacher', None, 'trailing', 0.5, 0.7, 'blurry') == dict(
        solver='ddim', spacing='trailing', eta=0.5, guidance_rescale=0.7, negative_prompt='blurry')
    for kw in (dict(teacher_sampler='ddim'), dict(teacher_spacing='trailing'), dict(teacher_eta=0.0), dict(guidance_rescale=0.5), dict(negative_prompt='x')):
        with pytest.raises(click.UsageError, match='--network teacher'):
            g.teacher_solver_options('snap.pkl', **kw)
    with pytest.raises(click.UsageError, match='--teacher_eta'):
        g.teacher_solver_options('teacher', 'dpmpp2m', None, 0.5)
    with pytest.raises(click.UsageError, match='--teacher_spacing'):
        g.teacher_solver_options('teacher', None, 'linspace')
    by = {p.name: p for p in g.main.params}
    for k in ('teacher_sampler', 'teacher_spacing', 'teacher_eta', 'guidance_rescale', 'negative_prompt'):
        assert by[k].default is None
    # refused by the command line before anything is loaded
    snap = tmp_path / 'network-snapshot.pkl'
    snap.write_bytes(b'x')
    common = ['--outdir', str(tmp_path / 'out'), '--seeds', '0-1', '--repo_id', 'random:tiny']
    for flag, value in (('--teacher_sampler', 'dpmpp2m'), ('--teacher_spacing', 'trailing'), ('--teacher_eta', '0.5'), ('--guidance_rescale', '0.7'),
                        ('--negative_prompt', 'blurry')):
        res = CliRunner().invoke(g.main, ['--network', str(snap), flag, value] + common)
        assert res.exit_code != 0 and flag in res.output and not os.path.exists(tmp_path / 'out')
    res = CliRunner().invoke(g.main, ['--network', 'teacher', '--teacher_sampler', 'dpmpp2m', '--teacher_eta', '0.5'] + common)
    assert res.exit_code != 0 and '--teacher_eta' in res.output and not os.path.exists(tmp_path / 'out')
    res = CliRunner().invoke(g.main, ['--network', 'teacher', '--teacher_sampler', 'dpmpp2m', '--init_images', str(tmp_path)] + common)
    assert res.exit_code != 0 and '--init_images' in res.output


# ---- the entry points ---------------------------------------------------------------------------------------------------------------------
def test_solver_entry_points_are_declared_and_forward_only():
    from sid_lsg_amd import ops
    from sid_lsg_amd._lib import parse_header
    from sid_lsg_amd.csrc.build import SOURCES
    from sid_lsg_amd.sd_util import teacher_sample_solver
    protos = parse_header()
    want = [ctypes.c_void_p] * 11 + [ctypes.c_int] * 6 + [ctypes.c_float, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    assert protos['sidlsg_solver_step'] == want and protos['sidlsg_solver_step_f32'] == want
    assert protos['sidlsg_cfg_rescale_stats'] == [ctypes.c_void_p] * 2 + [ctypes.c_int] * 4 + [ctypes.c_float] * 2 + [ctypes.c_void_p]
    assert 'solver.hip' in SOURCES
    x = torch.zeros(1, 4, 2, 2, requires_grad=True)
    e = torch.zeros(1, 4, 8)
    s = torch.ones(1)
    with pytest.raises(RuntimeError, match='forward only'):
        ops.solver_step(e, x, s, s, torch.zeros(1, 4), 1.0)
    with pytest.raises(RuntimeError, match='forward only'):
        ops.cfg_rescale_stats(torch.zeros(2, 4, 8, requires_grad=True), 4, 2.0, 0.7)
    p = inspect.signature(teacher_sample_solver).parameters
    assert list(p) == ['unet', 'latents', 'contexts', 'noise_scheduler', 'text_encoder', 'tokenizer', 'resolution', 'guidance_scale',
                       'num_inference_steps', 'return_images', 'vae', 'schedule_config', 'solver', 'spacing', 'eta', 'guidance_rescale',
                       'negative_contexts', 'randn']
    assert p['solver'].default == 'dpmpp2m' and p['spacing'].default is None and p['eta'].default == 0.0
    assert p['guidance_rescale'].default == 0.0 and p['negative_contexts'].default is None and p['randn'].default is None
    with pytest.raises(TypeError, match='HipUNet2DCondition'):
        teacher_sample_solver(torch.nn.Linear(1, 1), torch.zeros(1, 4, 8, 8), ['x'], None, None, None, 64)


def test_evaluate_teacher_routes_the_solver_options(monkeypatch):
    """With any solver option the metrics' G is teacher_sample_solver with those keywords and the report carries the long name; with
    none it is teacher_sample and the name it has always had.  (The model, the samplers and the metric are stand-ins: no device.)"""
    from sid_lsg_amd import metrics, sd_util
    from sid_lsg_amd import training_loop as tl
    calls, reported = [], []

    class Net:
        def eval(self):
            return self

        def requires_grad_(self, flag):
            return self
    monkeypatch.setattr(tl, 'load_sd15', lambda **kw: (Net(), 'vae', 'sched', 'te', 'tok'))
    monkeypatch.setattr(sd_util, 'teacher_sample_solver', lambda **kw: calls.append(('solver', kw)) or 'images')
    monkeypatch.setattr(sd_util, 'teacher_sample', lambda **kw: calls.append(('ddim', kw)) or 'images')

    def calc_metric(metric, G, **kw):
        assert G('z', ['a prompt'], init_timesteps=None) == 'images'
        return dict(metric=metric)
    monkeypatch.setattr(metrics, 'calc_metric', calc_metric)
    monkeypatch.setattr(metrics, 'report_metric', lambda result, run_dir, snapshot_pkl: reported.append(snapshot_pkl))
    common = dict(run_dir=None, dataset_kwargs=dict(class_name='x'), network_kwargs={}, device='cpu', metrics=['fid_test'], init_timestep=625,
                  metric_pt_path=None, metric_open_clip_path=None, pretrained_model_name_or_path='random:tiny', resolution=64,
                  teacher_steps=4, teacher_cfg=2.0)
    tl.evaluate_teacher(**common)
    tl.evaluate_teacher(teacher_sampler='dpmpp2m', teacher_spacing='trailing', teacher_rescale=0.7, **common)
    tl.evaluate_teacher(teacher_eta=0.5, **common)
    assert reported == ['teacher-ddim4-cfg2', 'teacher-dpmpp2m4-trailing-rs0.7-cfg2', 'teacher-ddim4-eta0.5-cfg2']
    assert [c[0] for c in calls] == ['ddim', 'solver', 'solver']
    new = ('solver', 'spacing', 'eta', 'guidance_rescale')
    assert not any(k in calls[0][1] for k in new)
    assert {k: calls[1][1][k] for k in new} == dict(solver='dpmpp2m', spacing='trailing', eta=0.0, guidance_rescale=0.7)
    assert {k: calls[2][1][k] for k in new} == dict(solver='ddim', spacing=None, eta=0.5, guidance_rescale=0.0)
    for _, kw in calls:
        assert kw['guidance_scale'] == 2.0 and kw['num_inference_steps'] == 4 and kw['return_images'] is True and kw['latents'] == 'z'
