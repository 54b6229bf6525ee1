"""Multi-process gradient-exchange tests on the GPU box (INTEGRATION.md mode 2).

The box has ONE GPU: the ranks of a 2-process run share cuda:0.  gloo carries the exchange where two ranks are needed;
RCCL ('nccl') is exercised for real at world size 1 (every collective of FlatGradReducer runs on the communication stream
against the compute / weight-gradient streams) and ATTEMPTED at world size 2 on the shared device -- RCCL either accepts it
or refuses duplicate devices, and the test records which."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from sid_lsg_amd._lib import lib
    lib.load()
    return torch.device('cuda:0')


def free_port():
    """A port the OS hands out as free right now (no fixed rendezvous port: back-to-back runs collide in TIME_WAIT)."""
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def launch(nproc, *worker_args, timeout=600):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(nproc), '--master-addr', '127.0.0.1',
           '--master-port', str(free_port()), os.path.join(HERE, 'mp_ddp_worker.py'), *worker_args]
    return subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout)


def test_ddp_wrapper_is_honoured_as_exchange_marker(dev, tmp_path):
    """Mode 2 of INTEGRATION.md with the DDP half: the reference passes the DistributedDataParallel WRAPPER of fake_score / G
    into the glue (sid_training_loop.py:416-421, 494-499) and runs all accumulation rounds but the last under `no_sync`
    (torch_utils/misc.py:168-175).  After the backward of the last round every rank's flat gradient buffer must hold the MEAN
    over ranks of the locally accumulated gradients -- and the exchange must have waited for the weight-gradient stream."""
    out = str(tmp_path / 'ddp')
    res = launch(2, 'ddp', out)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    for rank in (0, 1):
        r = np.load(f'{out}.rank{rank}.npz')
        print(f"rank {rank}: exchange error {float(r['err']):.2e}, local-vs-mean {float(r['local_vs_mean']):.2e}, losses {r['losses']}")
        assert bool(r['same_weights']), "DDP's constructor broadcast did not reach the flat buffer"
        assert float(r['local_vs_mean']) > 1e-3, 'the ranks must have different local gradients for this test to mean anything'
        # two backward passes differ by the fp32-atomics ordering noise only (test_weight_gradient_stream_changes_nothing)
        assert float(r['err']) < 2e-5
    assert float(np.load(f'{out}.rank1.npz')['moved']) > 0, 'rank 1 started from different weights and must have received rank 0\'s'


def _check_nccl(out, world):
    for rank in range(world):
        r = np.load(f'{out}.rank{rank}.npz')
        assert str(r['backend']) == 'nccl' and int(r['world']) == world
        print({k: (r[k].tolist() if r[k].ndim else float(r[k])) for k in r.files if k not in ('backend',)})
        assert sorted(r['fp32_fired'].tolist()) == [0, 1, 2, 3, 4]      # up + head, mid, down blocks 3 / 2 / 1 (grad_segments, round 5)
        assert float(r['fp32_whole']) <= 1e-7 * world          # fp32 sum of `world` equal-magnitude terms
        assert float(r['fp32_segments']) < 2e-5                # + atomics ordering noise of a second backward pass
        assert float(r['bf16_whole']) < 6e-3 and float(r['bf16_segments']) < 6e-3     # 2^-8 staging rounding


def test_flat_grad_reducer_on_rccl_world1(dev, tmp_path):
    """The production exchange path on backend 'nccl' (= RCCL): whole-buffer start()/wait(), marker-driven start_range()
    during the backward, the bf16 staging variant -- one rank, collectives forced (min_world=1), so the communication
    stream, its waits on the compute + weight-gradient streams and RCCL's own launch path all run on the real backend."""
    out = str(tmp_path / 'nccl1')
    res = launch(1, 'nccl', out)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    _check_nccl(out, 1)


def test_rccl_two_ranks_sharing_one_gpu(dev, tmp_path):
    """Two RCCL ranks on the SAME device.  If RCCL accepts that, the 2-rank results are checked like the 1-rank ones; if it
    refuses (duplicate device), the refusal is the expected outcome on a one-GPU box and its text is printed -- the 8-GPU run
    is the driver's (README: no scaling curve exists until SCALE runs)."""
    out = str(tmp_path / 'nccl2')
    res = launch(2, 'nccl', out, timeout=300)
    if res.returncode == 0:
        _check_nccl(out, 2)
        print('RCCL accepted two ranks on one device')
        return
    text = res.stdout + res.stderr
    known = ('Duplicate GPU detected', 'invalid usage', 'ncclInvalidUsage', 'ncclUnhandledCudaError', 'ncclSystemError', 'unhandled cuda error',
             'NCCL error', 'hipIpc')
    hit = [k for k in known if k in text]
    lines = [ln for ln in text.splitlines() if any(k in ln for k in known)][:6]
    print('RCCL refused two ranks on one device:\n' + '\n'.join(lines))
    assert hit, 'unexpected failure (not an RCCL refusal):\n' + text[-3000:]


def test_rccl_collectives_inside_the_captured_iteration(dev, tmp_path):
    """The HIP-graphed iteration with the gradient exchange in it: RCCL all-reduces (world 1, forced) are captured on the
    communication stream together with the compute / teacher / weight-gradient streams and replayed; losses and weights
    must equal the eager run's."""
    out = str(tmp_path / 'graph')
    res = launch(1, 'graph', out)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    r = np.load(f'{out}.rank0.npz')
    rel = np.abs(r['eager'] - r['graph']) / np.abs(r['eager'])
    print(f"eager {r['eager']} graph {r['graph']} max weight difference G {float(r['dG']):.2e} psi {float(r['dpsi']):.2e}")
    assert int(r['ngraphs']) == 1 and rel.max() < 2e-4
    assert max(float(r['dG']), float(r['dpsi'])) <= 2.01 * float(r['lr']) * int(r['iters'])


def _run_bench(nproc, *flags, env_extra=None, timeout=1500):
    import json
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0', **(env_extra or {}))
    root = os.path.dirname(HERE)
    if nproc == 1:
        cmd = [sys.executable, os.path.join(root, 'bench.py'), '--gpus', '1', *flags]
    else:
        cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(nproc), '--master-addr', '127.0.0.1',
               '--master-port', str(free_port()), os.path.join(root, 'bench.py'), '--gpus', str(nproc), *flags]
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout, cwd=root)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, f'exactly ONE JSON line from rank 0, got {len(lines)}'
    return json.loads(lines[0])


def test_bench_under_torchrun_two_ranks(dev):
    """The driver's scaling run: `python -m torch.distributed.run --nproc-per-node N bench.py --gpus N ...`.  Two ranks share
    one GPU (SIDLSG_BENCH_SHARE_GPU=1: gloo carries the exchange), --full and default flags otherwise -- per-family
    kernel timing on, i.e. including the extra `isolated` iterations after the timed region, which exchange gradients and
    therefore must be executed by every rank (a rank-0-only version of them paired rank 0's gradient all-reduce with the
    other ranks' timing all-reduce).  One JSON line, whole-job images/s, all ranks exit cleanly."""
    import json
    # (a small network: gloo moves the 2 x 3.4 GB of SD1.5 gradients through the host at ~40 s per iteration)
    out = _run_bench(2, '--steps', '2', '--warmup', '1', '--batch-gpu', '2', '--arch', 'tiny40', '--resolution', '128', '--full',
                     env_extra=dict(SIDLSG_BENCH_SHARE_GPU='1'))
    print({k: out[k] for k in ('value', 'n_gpus', 'ms_per_step', 'config')})
    assert out['n_gpus'] == 2 and out['steps'] == 2 and out['config']['global_batch'] == 4 and out['config']['parallelism'] == 'dp2'
    assert abs(out['value'] - 2 * 4 / (2 * out['ms_per_step'] / 1e3)) < 1e-4 * out['value']      # (the line carries 4 decimals)
    assert 'cpu_baseline' not in out                    # rank 0 at N = 1 only
    assert out['roofline']['launches_timed'] > 0 and out['roofline']['isolated_frac'] > 0 and out['teacher_pass']['ms'] > 0
    assert len(json.dumps(out)) < 4096, 'the driver keeps ~8 KB of stdout: the bench line must stay small'
    for k in ('loss_fake', 'loss_G'):
        assert np.isfinite(out[k])
    # the exposed-communication diagnosis a multi-GPU run must carry
    c = out['comm']
    print('comm:', c)
    assert set(c['exposed_ms_per_step']) == {'fake_score', 'G'} and c['comm_exposed_ms'] >= 0
    assert c['messages_per_step'] >= 2 and c['bytes_per_step'] > 0 and c['allreduce_algbw_GBps'] > 0 and c['backend'] == 'gloo'
    assert out['loss_check'] in ('ok', 'no reference stored for this configuration')


def test_bench_dump_outputs_are_reproducible(dev, tmp_path):
    """`bench.py --dump-outputs DIR`: two runs with the same arguments draw the same inputs, so what their last timed steps computed
    (losses, sampled weights and Adam second moments) agrees up to the bf16 path's run-to-run spread; the
    files are float32 / float64, under 64 MB, and the dumped losses are the ones the JSON line reports."""
    flags = ('--steps', '3', '--warmup', '1', '--batch-gpu', '2', '--arch', 'tiny40', '--resolution', '128', '--no-cpu-baseline',
             '--no-kernel-timing')
    runs = []
    for i in range(2):
        d = tmp_path / f'dump{i}'
        out = _run_bench(1, *flags, '--dump-outputs', str(d), env_extra=dict(SIDLSG_BENCH_DETAIL=str(tmp_path / f'detail{i}.json')))
        assert out['steps'] == 3 and out['ms_per_step'] > 0
        files = sorted(os.listdir(d))
        arrays = {f[:-len('.npy')]: np.load(d / f) for f in files}
        assert all(f.endswith('.npy') for f in files) and sum(os.path.getsize(d / f) for f in files) <= 64 << 20
        assert all(a.dtype in (np.float32, np.float64) and a.size > 0 and np.isfinite(a).all() for a in arrays.values())
        for k in ('loss_fake', 'loss_G'):
            assert abs(float(arrays[k][0]) - out[k]) <= 1e-4 * max(1.0, abs(out[k])), k      # (the line carries 4 decimals)
        runs.append(arrays)
    a, b = runs
    assert set(a) == set(b) == {'loss_fake', 'loss_G', 'G_params', 'fake_score_params', 'G_ema_params', 'G_adam_exp_avg_sq',
                                'fake_score_adam_exp_avg_sq', 'sample_index'}
    np.testing.assert_array_equal(a['sample_index'], b['sample_index'])
    for k in ('loss_fake', 'loss_G'):
        np.testing.assert_allclose(b[k], a[k], rtol=1e-3, err_msg=k)
    # (bf16 run-to-run spread, bench.dump_outputs; two full-size runs on two boxes met this bound, tiny40 runs were bit-equal)
    for k in ('G_params', 'fake_score_params', 'G_ema_params', 'G_adam_exp_avg_sq', 'fake_score_adam_exp_avg_sq'):
        print(f'{k}: max |difference| {np.abs(b[k] - a[k]).max():.3g} of max |value| {np.abs(a[k]).max():.3g}')
        np.testing.assert_allclose(b[k], a[k], rtol=1e-2, atol=1e-3 * float(np.abs(a[k]).max()), err_msg=k)


def test_bench_plain_run_leaves_the_extras_to_full(dev, tmp_path):
    """A plain `bench.py` run does only what its headline figure needs: set-up, warm-up, the timed steps and the line, with the
    per-family kernel figures sampled inside the timed region.  The loss check, the stand-alone (`isolated`) kernel figures, the
    teacher-pass timing and the CPU baseline come with --full, which prints the same kind of line."""
    flags = ('--steps', '2', '--warmup', '1', '--batch-gpu', '2', '--arch', 'tiny40', '--resolution', '128')
    plain = _run_bench(1, *flags, env_extra=dict(SIDLSG_BENCH_DETAIL=str(tmp_path / 'plain.json')))
    full = _run_bench(1, *flags, '--full', env_extra=dict(SIDLSG_BENCH_DETAIL=str(tmp_path / 'full.json')))
    for out in (plain, full):
        assert out['steps'] == 2 and out['warmup'] == 1 and out['n_gpus'] == 1 and out['unit'] == 'images/s' and out['higher_is_better']
        assert abs(out['value'] - 2 * 2 / (2 * out['ms_per_step'] / 1e3)) < 1e-4 * out['value']
        assert out['roofline']['launches_timed'] > 0 and np.isfinite(out['loss_fake']) and np.isfinite(out['loss_G'])
    assert plain['metric'] == full['metric'] and plain['dtype'] == full['dtype']
    for k in ('loss_check', 'teacher_pass', 'cpu_baseline'):
        assert k not in plain and k in full, k
    assert plain['roofline']['isolated_frac'] is None and full['roofline']['isolated_frac'] > 0
    assert full['teacher_pass']['ms'] > 0 and full['cpu_baseline']['value'] > 0


def test_rccl_world1_timing_of_the_full_size_messages(dev, tmp_path):
    """The exchange of one full-size network (859.5 M fp32 gradients = 4 messages of 0.86 GB) through RCCL at world size 1
    (collectives forced): message count / bytes / rate and the exposed wait as FlatGradReducer reports them -- the figures
    `bench.py --gpus N` prints as `comm`.  World 1 proves the plumbing and the reporting, not xGMI bandwidth."""
    out = str(tmp_path / 'msg')
    res = launch(1, 'messages', out)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    r = np.load(f'{out}.rank0.npz')
    print({k: r[k].tolist() for k in r.files})
    assert int(r['messages']) == 4 and int(r['bytes']) >= 859_520_964 * 4 and float(r['algbw_GBps']) > 0
    assert float(r['exposed_ms']) > 0 and float(r['comm_ms']) > 0 and bool(r['unchanged'])
