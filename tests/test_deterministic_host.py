"""Deterministic mode, host side (no GPU): the C switch, the ops policy, the command-line option and tools/compare_dumps.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def lib_det():
    from sid_lsg_amd._lib import LIB_PATH, lib
    if not os.path.isfile(LIB_PATH):
        from sid_lsg_amd.csrc.build import build
        build(verbose=False)
    lib.load()
    old = lib.sidlsg_set_deterministic.raw(-1)
    yield lib.sidlsg_set_deterministic.raw
    lib.sidlsg_set_deterministic.raw(old)


def test_c_switch_round_trips(lib_det):
    # a fresh process without SIDLSG_DETERMINISTIC starts with the mode off
    code = 'from sid_lsg_amd._lib import lib; lib.load(); print(lib.sidlsg_set_deterministic.raw(-1))'
    env = {k: v for k, v in os.environ.items() if k != 'SIDLSG_DETERMINISTIC'}
    for val, want in ((None, '0'), ('0', '0'), ('1', '1')):
        e = dict(env) if val is None else dict(env, SIDLSG_DETERMINISTIC=val)
        r = subprocess.run([sys.executable, '-c', code], cwd=ROOT, env=e, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert r.stdout.strip().splitlines()[-1] == want
    lib_det(0)
    assert lib_det(-1) == 0 and lib_det(-1) == 0         # -1 queries without changing the value
    assert lib_det(1) == 0                                # returns the previous setting
    assert lib_det(-1) == 1
    assert lib_det(0) == 1 and lib_det(-1) == 0


def test_ops_policy_explicit_then_env_then_torch(lib_det, monkeypatch):
    from sid_lsg_amd import ops
    old_explicit, old_env, old_torch = ops._det_explicit, ops._det_env, torch.are_deterministic_algorithms_enabled()
    try:
        monkeypatch.setattr(ops, '_det_env', False)
        torch.use_deterministic_algorithms(False)
        assert ops.set_deterministic(None) is False and lib_det(-1) == 0
        # the torch flag alone switches it on -- and the value reaches the C flag at the next backward / column sum
        torch.use_deterministic_algorithms(True)
        assert ops.is_deterministic() is True
        assert ops.sync_deterministic() is True and lib_det(-1) == 1
        # an explicit setting wins over the torch flag
        assert ops.set_deterministic(False) is False and lib_det(-1) == 0
        torch.use_deterministic_algorithms(False)
        # the environment variable wins over the torch flag when nothing is set explicitly
        monkeypatch.setattr(ops, '_det_env', True)
        assert ops.set_deterministic(None) is True and lib_det(-1) == 1
        assert ops.set_deterministic(False) is False and lib_det(-1) == 0
        monkeypatch.setattr(ops, '_det_env', False)
        ops.set_deterministic(None)
        with ops.deterministic():
            assert ops.is_deterministic() and lib_det(-1) == 1
            with ops.deterministic(False):
                assert not ops.is_deterministic() and lib_det(-1) == 0
            assert lib_det(-1) == 1
        assert ops._det_explicit is None and lib_det(-1) == 0
        with pytest.raises(ValueError):
            ops.set_deterministic(1)
    finally:
        torch.use_deterministic_algorithms(old_torch)
        ops._det_env = old_env
        ops.set_deterministic(old_explicit)


def test_every_ops_backward_syncs_the_mode():
    from sid_lsg_amd import ops
    fns = [c for c in vars(ops).values() if isinstance(c, type) and issubclass(c, torch.autograd.Function) and c.__module__ == ops.__name__
           and 'backward' in c.__dict__]
    assert len(fns) > 10
    for c in fns:
        assert c.__dict__['backward'].__func__.__wrapped__ is not None, c.__name__


def test_sid_train_deterministic_option(tmp_path):
    from click.testing import CliRunner
    import sid_train
    (tmp_path / 'aesthetics_6_plus.txt').write_text('a prompt\n')
    base = ['--outdir', str(tmp_path / 'runs'), '--data_prompt_text', str(tmp_path), '--sd_model', 'random:tiny', '--seed', '3',
            '--batch', '8', '--batch-gpu', '2', '--duration', '0.01', '--dry-run']
    for extra, want in (([], False), (['--deterministic', '1'], True), (['--deterministic', '0'], False)):
        seen = {}
        orig = sid_train.build_config

        def spy(o):
            c = orig(o)
            seen['c'] = c
            return c
        sid_train.build_config = spy
        try:
            res = CliRunner().invoke(sid_train.main, base + extra)
        finally:
            sid_train.build_config = orig
        assert res.exit_code == 0, res.output
        c = seen['c']
        assert c.deterministic is want
        assert 'deterministic' not in c.network_kwargs
        assert c.network_kwargs == dict(use_fp16=False, compute_dtype='bf16', teacher_weights='bf16')
    # an options object without the key (older callers) still builds
    o = sid_train.EasyDict(dict(
        outdir='x', data=None, data_stat=None, data_prompt_text=str(tmp_path), duration=0.01, batch=8, batch_gpu=2, ema=0.05,
        xflip=0.0, bench=True, cache=True, workers=1, desc=None, nosubdir=False, tick=2, snap=50, dump=100, seed=3, transfer=None,
        resume=None, dry_run=True, metrics=None, sd_model='random:tiny', resolution=512, init_timestep=625, fp16=False, ls=1, lsg=1,
        alpha=1, tmax=980, tmin=20, lr=1e-6, glr=2e-6, train_mode=True, network_pkl=None, cfg_train_fake=1.5, cfg_eval_fake=1.5,
        cfg_eval_real=1.5, metric_pt_path=None, metric_clip_path=None, metric_open_clip_path=None, enable_xformers=True,
        gradient_checkpointing=False, optimizer='adam', num_steps=1, fake_score_use_lora=False))
    assert sid_train.build_config(o).deterministic is False


def test_training_loop_takes_deterministic():
    import inspect
    from sid_lsg_amd.training_loop import training_loop
    assert inspect.signature(training_loop).parameters['deterministic'].default is False


def _run_compare(a, b):
    return subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'compare_dumps.py'), str(a), str(b)],
                          capture_output=True, text=True, timeout=120)


def test_compare_dumps(tmp_path):
    a, b = tmp_path / 'a', tmp_path / 'b'
    a.mkdir(); b.mkdir()
    x = np.random.default_rng(0).standard_normal(1000).astype(np.float32)
    for d in (a, b):
        np.save(d / 'G_params.npy', x)
        np.save(d / 'loss_G.npy', np.array([0.25], np.float32))
    r = _run_compare(a, b)
    assert r.returncode == 0, r.stdout
    assert r.stdout.count(' bit-equal  ') == 2 and 'all files bit-equal' in r.stdout
    # one ulp in one element
    y = x.copy()
    y[17] = np.nextafter(y[17], np.float32(np.inf))
    np.save(b / 'G_params.npy', y)
    r = _run_compare(a, b)
    assert r.returncode != 0
    line = [ln for ln in r.stdout.splitlines() if ln.startswith('G_params.npy')][0]
    assert 'DIFFERENT' in line and '1 of 1000' in line and '1.000e-03' in line
    assert float(line.split('max|a-b| = ')[1].split()[0]) == pytest.approx(abs(float(y[17]) - float(x[17])), rel=1e-3)
    # a file only one side has
    np.save(b / 'G_params.npy', x)
    np.save(a / 'extra.npy', x)
    r = _run_compare(a, b)
    assert r.returncode != 0 and 'MISSING' in r.stdout
