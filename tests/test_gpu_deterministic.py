"""Deterministic mode (include/sidlsg_hip.h sidlsg_set_deterministic, ops.set_deterministic): every reduction that used fp32 atomics
repeats bit for bit on shapes that take the atomic path in the default mode, and stays within the op tests' tolerance of fp32 torch;
the tiny40 training step and the command line repeat bit for bit."""
import glob
import os
import pickle
import socket
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16, F32 = torch.bfloat16, torch.float32
REPEATS = 8


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs an MI355X')
    from sid_lsg_amd import ops
    ops.ensure_workspace('cuda')
    return torch.device('cuda')


@pytest.fixture
def det(dev):
    from sid_lsg_amd import ops
    old = ops._det_explicit
    ops.set_deterministic(True)
    assert ops.lib.sidlsg_set_deterministic.raw(-1) == 1
    yield
    ops.set_deterministic(old)


def _p(t):
    return None if t is None else t.data_ptr()


def _s():
    return torch.cuda.current_stream().cuda_stream


def _repeat(run, n=REPEATS):
    """run() -> tuple of fresh output tensors; all n runs must be bit-equal.  Returns the first."""
    first = None
    for _ in range(n):
        out = tuple(t.clone() for t in run())
        torch.cuda.synchronize()
        if first is None:
            first = out
        else:
            for a, b in zip(first, out):
                assert torch.equal(a, b), 'deterministic mode: two runs differ'
    return first


def _close(a, ref, rtol=2e-3, atol=1e-3):
    torch.testing.assert_close(a.double(), ref.double(), rtol=rtol, atol=atol * float(ref.abs().max()) + 1e-6)


# ---- column sums ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', [320, 1280])
@pytest.mark.parametrize('dtype', [BF16, F32])
def test_colsum_repeats(dev, det, N, dtype):
    from sid_lsg_amd._lib import lib
    B, rows = 16, 4096
    g = torch.randn(B * rows, N, device=dev).to(dtype)
    fn = lib.sidlsg_colsum if dtype == BF16 else lib.sidlsg_colsum_f32
    sfn = lib.sidlsg_colsum_strided if dtype == BF16 else lib.sidlsg_colsum_strided_f32

    def run():
        pb, tot = torch.zeros(B, N, device=dev), torch.full((N,), 0.5, device=dev)
        fn(_p(g), N, _p(pb), _p(tot), None, B, rows, N, _s())
        wide = torch.zeros(B, N + 64, device=dev)
        tot2 = torch.zeros(N, device=dev)
        sfn(_p(g), N, wide.data_ptr() + 32 * 4, N + 64, _p(tot2), B, rows, N, _s())
        return pb, tot, wide, tot2
    pb, tot, wide, tot2 = _repeat(run)
    ref = g.double().view(B, rows, N).sum(1)
    _close(pb, ref)
    _close(tot - 0.5, ref.sum(0))
    assert torch.equal(wide[:, 32:32 + N], pb)         # the strided entry point: same sums into a wider buffer
    _close(tot2, ref.sum(0))
    assert not wide[:, :32].any() and not wide[:, 32 + N:].any()


def test_colsum_without_workspace_is_order_fixed(dev, det):
    from sid_lsg_amd._lib import lib
    from sid_lsg_amd import ops
    B, rows, N = 4, 1024, 320
    g = torch.randn(B * rows, N, device=dev).to(BF16)
    ws = ops.ensure_workspace(dev)
    lib.sidlsg_set_workspace(None, 0)
    try:
        def run():
            pb, tot = torch.zeros(B, N, device=dev), torch.zeros(N, device=dev)
            lib.sidlsg_colsum(_p(g), N, _p(pb), _p(tot), None, B, rows, N, _s())
            return pb, tot
        pb, tot = _repeat(run, 3)
    finally:
        torch.cuda.synchronize()
        lib.sidlsg_set_workspace(ws.data_ptr(), ws.numel() * 4)
    ref = g.double().view(B, rows, N).sum(1)
    _close(pb, ref)
    _close(tot, ref.sum(0))


# ---- LayerNorm / GroupNorm parameter gradients -------------------------------------------------------------------------------
def _ln(dev, rows, C):
    from sid_lsg_amd._lib import lib
    x = torch.randn(rows, C, device=dev).to(BF16)
    dy = torch.randn(rows, C, device=dev).to(BF16)
    gamma, beta = 1 + 0.1 * torch.randn(C, device=dev), 0.1 * torch.randn(C, device=dev)
    y, stats = torch.empty_like(x), torch.empty(rows, 2, device=dev)
    lib.sidlsg_layernorm_fwd(_p(x), _p(gamma), _p(beta), _p(y), _p(stats), rows, C, 1e-5, _s())
    ws = torch.empty(lib.sidlsg_layernorm_bwd_nblocks.raw(rows) * C * 2, device=dev)
    return x, dy, gamma, beta, stats, ws


def test_layernorm_backward_repeats_and_deferred_equals_immediate(dev, det):
    from sid_lsg_amd._lib import lib
    rows, C = 65536, 320
    x, dy, gamma, beta, stats, ws = _ln(dev, rows, C)

    def run(defer):
        dx, dg, db = torch.empty_like(x), torch.zeros(C, device=dev), torch.zeros(C, device=dev)
        h = _s()
        if defer:
            assert lib.sidlsg_defer_reductions.raw(h, 1) >= 0
        lib.sidlsg_layernorm_bwd(_p(x), _p(dy), _p(stats), _p(gamma), None, _p(dx), _p(dg), _p(db), _p(ws), rows, C, h)
        if defer:
            assert lib.sidlsg_pending_reductions.raw(h) == 1
            assert lib.sidlsg_defer_reductions.raw(h, 0) >= 0      # flush (returns the number of jobs run) + forget
        return dx, dg, db
    imm = _repeat(lambda: run(False))
    dfr = _repeat(lambda: run(True))
    for a, b in zip(imm, dfr):
        assert torch.equal(a, b), 'deferred and immediate reductions differ'
    xr = x.double()
    xh = (xr - xr.mean(1, keepdim=True)) / torch.sqrt(xr.var(1, unbiased=False, keepdim=True) + 1e-5)
    _close(imm[1], (dy.double() * xh).sum(0))
    _close(imm[2], dy.double().sum(0))


def _gn_case(dev, B, HW, C, G, silu=1):
    from sid_lsg_amd._lib import lib
    x = torch.randn(B, HW, C, device=dev).to(BF16)
    dy = torch.randn(B, HW, C, device=dev).to(BF16)
    gamma, beta = 1 + 0.1 * torch.randn(C, device=dev), 0.1 * torch.randn(C, device=dev)
    ws = torch.empty(lib.sidlsg_groupnorm_ws_floats.raw(B, HW, C, G), device=dev)
    y, stats = torch.empty_like(x), torch.empty(B, G, 2, device=dev)
    lib.sidlsg_groupnorm_fwd(_p(x), _p(gamma), _p(beta), _p(y), _p(stats), _p(ws), B, HW, C, G, 1e-5, silu, _s())

    def run():
        dx, dg, db = torch.empty_like(x), torch.zeros(C, device=dev), torch.zeros(C, device=dev)
        lib.sidlsg_groupnorm_bwd(_p(x), _p(dy), _p(stats), _p(gamma), _p(beta), None, _p(dx), _p(dg), _p(db), _p(ws), B, HW, C, G, silu, _s())
        return dx, dg, db
    dx, dg, db = _repeat(run)
    # fp32 torch reference of dgamma / dbeta
    xr = x.double().view(B, HW, G, C // G)
    xh = ((xr - xr.mean((1, 3), keepdim=True)) / torch.sqrt(xr.var((1, 3), unbiased=False, keepdim=True) + 1e-5)).view(B, HW, C)
    d = dy.double()
    if silu:
        z = xh * gamma.double() + beta.double()
        s = torch.sigmoid(z)
        d = d * s * (1 + z * (1 - s))
    _close(dg, (d * xh).sum((0, 1)))
    _close(db, d.sum((0, 1)))


@pytest.mark.parametrize('HW,C', [(256, 1280), (64, 1280), (4096, 320)])     # 16x16 and 8x8 one-pass stages, 64x64 two-kernel path
def test_groupnorm_backward_repeats(dev, det, HW, C):
    _gn_case(dev, 16, HW, C, 32)


_GN_GROUP_SCRIPT = r'''
import sys, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests')
import test_gpu_deterministic as t
from sid_lsg_amd import ops
ops.ensure_workspace('cuda'); ops.set_deterministic(True)
t._gn_case(torch.device('cuda'), 16, 1024, 640, 32)
t._gn_case(torch.device('cuda'), 16, 1024, 1280, 32, silu=0)
print('ok')
'''


def test_groupnorm_group_kernels_repeat(dev):
    env = dict(os.environ, SIDLSG_GN_GROUP='7')
    r = subprocess.run([sys.executable, '-c', _GN_GROUP_SCRIPT, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith('ok'), r.stdout[-2000:] + r.stderr[-4000:]


# ---- weight gradients --------------------------------------------------------------------------------------------------------
def test_dense_wgrad_with_bias_repeats(dev, det):
    from sid_lsg_amd._lib import lib
    from sid_lsg_amd.ops import _WgJob
    import ctypes
    M, N, K = 65536, 320, 320
    dy = torch.randn(M, N, device=dev).to(BF16)
    a = torch.randn(M, K, device=dev).to(BF16)
    ref_w = dy.float().t() @ a.float()
    ref_b = dy.double().sum(0)

    def single():
        dw, db = torch.zeros(N, K, device=dev), torch.zeros(N, device=dev)
        lib.sidlsg_wgrad_bf16(_p(dy), N, _p(a), K, _p(dw), _p(db), M, N, K, _s())
        return dw, db

    def grouped():
        dws = [torch.zeros(N, K, device=dev) for _ in range(2)]
        dbs = [torch.zeros(N, device=dev) for _ in range(2)]
        arr = (_WgJob * 2)()
        for i in range(2):
            arr[i].dY, arr[i].A, arr[i].dW, arr[i].dBias = _p(dy), _p(a), _p(dws[i]), _p(dbs[i])
            arr[i].ldy, arr[i].lda, arr[i].M, arr[i].N, arr[i].K, arr[i].assign = N, K, M, N, K, i
        lib.sidlsg_wgrad_group_bf16(ctypes.addressof(arr), 2, _s())
        return dws[0], dbs[0], dws[1], dbs[1]
    dw, db = _repeat(single)
    g = _repeat(grouped)
    for w, b in ((dw, db), g[:2], g[2:]):
        _close(w, ref_w, rtol=1e-2, atol=2e-3)
        _close(b, ref_b)


def test_conv_wgrad_with_bias_repeats(dev, det):
    from sid_lsg_amd._lib import lib
    B, H, W, Cin, Cout = 16, 32, 32, 320, 320
    x = torch.randn(B, H, W, Cin, device=dev).to(BF16)
    dy = torch.randn(B, H, W, Cout, device=dev).to(BF16)

    def run():
        dw, db = torch.zeros(Cout, 3, 3, Cin, device=dev), torch.zeros(Cout, device=dev)
        lib.sidlsg_conv3x3_wgrad_bf16(_p(dy), Cout, _p(x), Cin, _p(dw), _p(db), B, H, W, Cin, Cout, 1, 0, _s())
        return dw, db
    dw, db = _repeat(run)
    xr = x.float().permute(0, 3, 1, 2)
    dyr = dy.float().permute(0, 3, 1, 2)
    ref = torch.nn.grad.conv2d_weight(xr, (Cout, Cin, 3, 3), dyr, padding=1).permute(0, 2, 3, 1)
    _close(dw, ref, rtol=1e-2, atol=2e-3)
    _close(db, dy.double().sum((0, 1, 2)))


def test_wgrad_without_workspace_repeats(dev, det):
    from sid_lsg_amd._lib import lib
    from sid_lsg_amd import ops
    M, N, K = 16384, 320, 320
    dy = torch.randn(M, N, device=dev).to(BF16)
    a = torch.randn(M, K, device=dev).to(BF16)
    ws = ops.ensure_workspace(dev)
    lib.sidlsg_set_workspace(None, 0)
    try:
        def run():
            dw, db = torch.zeros(N, K, device=dev), torch.zeros(N, device=dev)
            lib.sidlsg_wgrad_bf16(_p(dy), N, _p(a), K, _p(dw), _p(db), M, N, K, _s())
            return dw, db
        dw, db = _repeat(run, 3)
    finally:
        torch.cuda.synchronize()
        lib.sidlsg_set_workspace(ws.data_ptr(), ws.numel() * 4)
    _close(dw, dy.float().t() @ a.float(), rtol=1e-2, atol=2e-3)
    _close(db, dy.double().sum(0))


def test_fp32_wgrad_pixel_split_repeats(dev, det):
    from sid_lsg_amd._lib import lib
    M, N, K = 16384, 320, 320          # 25 tiles -> ~20 pixel splits
    dy = torch.randn(M, N, device=dev)
    a = torch.randn(M, K, device=dev)

    def run():
        dw = torch.zeros(N, K, device=dev)
        lib.sidlsg_wgrad_f32(_p(dy), N, _p(a), K, _p(dw), None, M, N, K, _s())
        return (dw,)
    (dw,) = _repeat(run)
    _close(dw, dy.double().t() @ a.double(), rtol=1e-4, atol=1e-5)


# ---- the training step -------------------------------------------------------------------------------------------------------
def _assert_same(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        assert torch.equal(a[k], b[k]), f'{what}: {k} differs (max {float((a[k].double() - b[k].double()).abs().max()):.3e})'


@pytest.mark.parametrize('dtype', ['bf16', 'fp32'])
def test_step_repeats_bit_for_bit(dev, dtype, tmp_path):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from det_step_worker import run_step
    dt = F32 if dtype == 'fp32' else BF16
    ref = run_step(dt)
    _assert_same(ref, run_step(dt), 'a second in-process step')
    envs = [{'SIDLSG_WGRAD_STREAMS': '2'}, {'SIDLSG_DEFER_REDUCE': '0'}, {'SIDLSG_SEG_OPT': '1'}] if dtype == 'bf16' else [{}]
    for extra in envs:
        out = tmp_path / 'step.pt'
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'det_step_worker.py'), str(out), dtype],
                           env=dict(os.environ, **extra), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, f'{extra}: {r.stdout[-2000:]}{r.stderr[-4000:]}'
        _assert_same(ref, torch.load(out), f'worker with {extra}')


# ---- end to end: the command line, CLIP text encoder included -----------------------------------------------------------------
def _tensors(obj, prefix='', seen=None):
    """Every tensor with data reachable from obj (dicts, lists, modules and their attributes -- a snapshot network keeps its
    parameters in flat buffers), by path."""
    seen = set() if seen is None else seen
    if id(obj) in seen:
        return {}
    seen.add(id(obj))
    if isinstance(obj, torch.Tensor):
        return {} if obj.is_meta else {prefix: obj.detach().cpu()}
    if isinstance(obj, torch.nn.Module):
        obj = vars(obj)
    out = {}
    if isinstance(obj, dict):
        for k, v in obj.items():
            out.update(_tensors(v, f'{prefix}/{k}', seen))
    elif isinstance(obj, (list, tuple)):
        for i, v in enumerate(obj):
            out.update(_tensors(v, f'{prefix}/{i}', seen))
    return out


def _free_port():
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        return sk.getsockname()[1]


def test_cli_deterministic_runs_repeat(dev, tmp_path):
    (tmp_path / 'aesthetics_6_plus.txt').write_text('\n'.join(f'prompt number {i}' for i in range(40)) + '\n')
    runs, procs = [], []
    for r in range(2):          # the two runs side by side
        outdir = tmp_path / f'run{r}'
        cmd = [sys.executable, os.path.join(ROOT, 'sid_train.py'), '--outdir', str(outdir), '--nosubdir', '--data_prompt_text', str(tmp_path),
               '--sd_model', 'random:tiny', '--seed', '1', '--batch', '4', '--batch-gpu', '2', '--duration', '0.00004', '--ema', '0.00001',
               '--tick', '1', '--snap', '1', '--dump', '1', '--cfg_train_fake', '1.5', '--cfg_eval_fake', '1.5', '--cfg_eval_real', '1.5',
               '--resolution', '128', '--deterministic', '1']
        env = dict(os.environ, MASTER_PORT=str(_free_port()))        # each run is a world of one with its own rendezvous
        procs.append(subprocess.Popen(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
        runs.append(str(outdir))
    try:
        outs = [p.communicate(timeout=400) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for p, (so, se) in zip(procs, outs):
        assert p.returncode == 0, so[-3000:] + se[-3000:]
        assert 'Deterministic mode: on' in so
    for pattern in ('training-state-*.pt', 'network-snapshot-*.pkl'):
        files = [sorted(glob.glob(os.path.join(d, pattern))) for d in runs]
        assert files[0] and [os.path.basename(f) for f in files[0]] == [os.path.basename(f) for f in files[1]]
        for fa, fb in zip(*files):
            if fa.endswith('.pt'):
                a, b = torch.load(fa, map_location='cpu', weights_only=False), torch.load(fb, map_location='cpu', weights_only=False)
            else:
                with open(fa, 'rb') as f:
                    a = pickle.load(f)
                with open(fb, 'rb') as f:
                    b = pickle.load(f)
            ta, tb = _tensors(a), _tensors(b)
            assert len(ta) > 2 and ta.keys() == tb.keys()
            for k in ta:
                assert torch.equal(ta[k], tb[k]), f'{os.path.basename(fa)}{k} differs between two deterministic runs'
