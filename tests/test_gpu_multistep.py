"""Multi-step generator training (--num_steps N > 1) on the GPU: the fused step-boundary kernel (sidlsg_step_renoise), the N-step
training sampler against the reference's (tests/golden/glue_ns_tiny.npz), the product loop against the unmodified reference loop at
N = 2 / 4 (tests/golden/loop_ns*.npz), and the fast paths of the step at N = 2."""
import glob
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


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from sid_lsg_amd._lib import lib
    lib.load()
    return torch.device('cuda:0')


def _sched(pt):
    from sid_lsg_amd.scheduler import DDPMScheduler
    return DDPMScheduler(prediction_type=pt)


def _boundary_inputs(dev, B, H, W, seed=0):
    g = torch.Generator().manual_seed(seed)
    eps = torch.zeros(B, H * W, 8)
    eps[..., :4] = torch.randn(B, H * W, 4, generator=g)
    xt = torch.randn(B, 4, H, W, generator=g)
    noise = torch.randn(B, 4, H, W, generator=g)
    t0 = torch.randint(300, 980, (B,), generator=g)
    t1 = (t0 * 0.5).long()
    return eps.to(dev), xt.to(dev), noise.to(dev), t0.to(dev), t1.to(dev)


# ---- kernel ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pt', ['epsilon', 'v_prediction'])
@pytest.mark.parametrize('act', [BF16, F32])
@pytest.mark.parametrize('shape', [(3, 16, 16), (2, 9, 7)])
def test_step_renoise_forward_is_bit_equal_to_cfg_x0_then_noisy_input(dev, pt, act, shape):
    from sid_lsg_amd import ops
    sched = _sched(pt).to(dev)
    eps, xt, noise, t0, t1 = _boundary_inputs(dev, *shape)
    s0, s1 = sched.coefficients(t0)
    s0n, s1n = sched.coefficients(t1)
    xh = ops.cfg_x0(eps, xt, s0, s1, 1.0, True, act, prediction_type=pt)
    ref_in, ref_xt = ops.noisy_input(xh, noise, s0n, s1n, 1, act)
    out, xtn = ops.step_renoise(eps, xt, s0, s1, s0n, s1n, noise, act, prediction_type=pt)
    torch.cuda.synchronize()
    assert out.dtype == act and out.shape == ref_in.shape
    assert torch.equal(xtn, ref_xt), float((xtn - ref_xt).abs().max())
    assert torch.equal(out, ref_in)
    assert not out[..., 4:].any()


@pytest.mark.parametrize('pt', ['epsilon', 'v_prediction'])
@pytest.mark.parametrize('act', [F32, BF16])
def test_step_renoise_backward_matches_autograd(dev, pt, act):
    """d eps and d x_t of the fused backward against torch autograd of the fp64 formulas: 1e-6 relative in fp32 mode, bf16 rounding
    of d eps in bf16 mode.  Padding channels of d eps are zero."""
    from sid_lsg_amd import ops
    sched = _sched(pt).to(dev)
    eps, xt, noise, t0, t1 = _boundary_inputs(dev, 2, 12, 10, seed=1)
    s0, s1 = sched.coefficients(t0)
    s0n, s1n = sched.coefficients(t1)
    gen = torch.Generator().manual_seed(5)
    g_in = torch.randn(2, 12, 10, 8, generator=gen).to(dev)
    g_in[..., 4:] = 0
    g_in = g_in.to(act)
    g_xt = torch.randn(2, 4, 12, 10, generator=gen).to(dev)
    e = eps.clone().requires_grad_(True)
    x = xt.clone().requires_grad_(True)
    out, xtn = ops.step_renoise(e, x, s0, s1, s0n, s1n, noise, act, prediction_type=pt)
    torch.autograd.backward([out, xtn], [g_in, g_xt])
    torch.cuda.synchronize()
    # fp64 reference
    ed = eps.double().cpu().requires_grad_(True)
    xd = xt.double().cpu().requires_grad_(True)
    v = lambda a: a.double().cpu().view(-1, 1, 1, 1)  # noqa: E731
    en = ed[..., :4].permute(0, 2, 1).reshape(xt.shape)
    xh = (xd - v(s1) * en) / v(s0) if pt == 'epsilon' else v(s0) * xd - v(s1) * en
    xn = v(s0n) * xh + v(s1n) * noise.double().cpu()
    gi = g_in.double().cpu()[..., :4].permute(0, 3, 1, 2)
    (xn * gi).sum().add_((xn * g_xt.double().cpu()).sum()).backward()
    de, dx = e.grad, x.grad
    assert de.dtype == F32 and not de[..., 4:].any()
    rel = lambda a, b: float((a.double().cpu() - b).abs().max() / b.abs().max())  # noqa: E731
    # d eps is stored in the compute dtype (bf16 rounding); d x_t is fp32 arithmetic on the same g the reference uses in either mode
    assert rel(de, ed.grad) < (1e-6 if act == F32 else 8e-3), rel(de, ed.grad)
    assert rel(dx, xd.grad) < 1e-6, rel(dx, xd.grad)


def test_step_renoise_propagates_nan_and_rejects_bad_modes(dev):
    from sid_lsg_amd import ops
    from sid_lsg_amd._lib import lib
    sched = _sched('epsilon').to(dev)
    eps, xt, noise, t0, t1 = _boundary_inputs(dev, 2, 8, 8)
    eps[1, 5, 2] = float('nan')
    s0, s1 = sched.coefficients(t0)
    s0n, s1n = sched.coefficients(t1)
    out, xtn = ops.step_renoise(eps, xt, s0, s1, s0n, s1n, noise, BF16)
    xh = ops.cfg_x0(eps, xt, s0, s1, 1.0, True, BF16)
    ref_in, ref_xt = ops.noisy_input(xh, noise, s0n, s1n, 1, BF16)
    torch.cuda.synchronize()
    assert torch.isnan(xtn[1]).any() and not torch.isnan(xtn[0]).any()
    assert torch.equal(torch.isnan(xtn), torch.isnan(ref_xt)) and torch.equal(torch.isnan(out.float()), torch.isnan(ref_in.float()))
    p = lambda a: a.data_ptr()  # noqa: E731
    for mode in (0, 3):
        rc = lib.sidlsg_step_renoise.raw(p(eps), p(xt), p(s0), p(s1), p(s0n), p(s1n), p(noise), p(out), p(xtn), 2, 4, 64, 8, mode, None)
        assert rc != 0


# ---- glue -----------------------------------------------------------------------------------------------------------------------
def _rel(a, b):
    b = torch.as_tensor(b).double()
    return float((a.detach().double().cpu() - b).abs().max() / b.abs().max())


@pytest.mark.parametrize('cd', [F32, BF16])
def test_multistep_sampler_matches_reference_golden(dev, golden_dir, cd, monkeypatch):
    """sid_sd_sampler(train_sampler=True, num_steps=2 / 4) with the eps_i the reference drew, against the reference's x_hat and the
    gradients of <x_hat, w> on a few parameters (fp32 mode)."""
    from oracle import fixtures
    from sid_lsg_amd.sd_util import sid_sd_sampler
    from sid_lsg_amd.unet import CONFIGS, HipUNet2DCondition
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    g = np.load(os.path.join(golden_dir, 'glue_ns_tiny.npz'))
    prompts = [str(p) for p in g['prompts']]
    names = [str(n) for n in g['grad_names']]
    for p in ('eps', 'v'):
        pt = 'epsilon' if p == 'eps' else 'v_prediction'
        ref, _, _, te, tok = fixtures.factory('tiny')
        net = HipUNet2DCondition(CONFIGS['tiny'], compute_dtype=cd)
        net.prediction_type = pt
        net.materialize(dev, source=ref.state_dict())
        net.train().requires_grad_(True)
        sched = _sched(pt).to(dev)
        te = te.to(dev)
        params = dict(net.named_parameters())
        for n in (2, 4):
            k = f'{p}_ns{n}'
            z = torch.from_numpy(g[k + '_z']).to(dev)
            w = torch.from_numpy(g[k + '_w']).to(dev)
            drawn = [torch.from_numpy(e).to(dev) for e in g[k + '_eps']]
            assert len(drawn) == n - 1
            it = iter(drawn)
            monkeypatch.setattr(torch, 'randn_like', lambda *a, **kw: next(it))
            net.flat_grads.zero_()
            init_t = torch.full((len(z),), 625, dtype=torch.long, device=dev)
            xhat = sid_sd_sampler(net, z, prompts, init_t, sched, te, tok, 64, dtype=F32, num_steps=n, train_sampler=True)
            monkeypatch.undo()
            (xhat * w).sum().backward()
            torch.cuda.synchronize()
            e = _rel(xhat, g[k + '_xhat'])
            bound = 1e-5 if cd == F32 else n * 3e-2
            print(f'{k} {cd}: x_hat {e:.2e} (bound {bound})')
            assert e < bound, (k, e)
            if cd == F32:
                for name in names:
                    eg = _rel(params[name].grad, g[f'{k}_grad/{name}'])
                    print(f'   grad {name}: {eg:.2e}')
                    assert eg < 1e-4, (k, name, eg)


# ---- loop -----------------------------------------------------------------------------------------------------------------------
def _loop_kwargs(g, run_dir, pdir, dev, mode):
    from sid_lsg_amd.dnnlib_util import EasyDict
    kappa = [float(k) for k in g['kw_kappa']]
    bs = int(g['kw_batch_size'])
    return dict(run_dir=str(run_dir), network_kwargs=EasyDict(use_fp16=False, compute_dtype=mode),
                dataset_prompt_text_kwargs=EasyDict(class_name='sid_lsg_amd.data.PromptDataset', path=str(pdir),
                                                    resolution=int(g['kw_resolution']), prompt_only=True),
                fake_score_optimizer_kwargs=EasyDict(class_name='torch.optim.Adam', lr=float(g['kw_lr']), betas=[0.0, 0.999], eps=1e-8),
                g_optimizer_kwargs=EasyDict(class_name='torch.optim.Adam', lr=float(g['kw_glr']), betas=[0.0, 0.999], eps=1e-8),
                seed=int(g['kw_seed']), batch_size=bs, batch_gpu=int(g['kw_batch_gpu']), total_kimg=int(g['kw_iterations']) * bs / 1000.0,
                ema_halflife_kimg=50, kimg_per_tick=10 ** 9, snapshot_ticks=None, state_dump_ticks=None, alpha=float(g['kw_alpha']),
                tmax=980, tmin=20, device=dev, metrics=None, init_timestep=625, cfg_train_fake=kappa[0], cfg_eval_fake=kappa[1],
                cfg_eval_real=kappa[2], resolution=int(g['kw_resolution']), enable_xformers=False, rng_device='cpu',
                num_steps=int(g['num_steps']))


@pytest.mark.parametrize('mode', ['fp32', 'bf16'])
@pytest.mark.parametrize('name', ['ns2_k15_a1', 'ns4_k1_a12', 'v_ns2_k15_a1'])
def test_product_loop_matches_reference_multistep_golden(dev, golden_dir, tmp_path, name, mode):
    """training_loop(num_steps=N) against the unmodified reference loop at N = 2 / 4 (epsilon and v): fp32 mode 1e-3 relative on both
    losses at every iteration; bf16 the bounds of tests/test_gpu_unet.py::test_product_loop_matches_reference_golden."""
    from oracle import fixtures
    from sid_lsg_amd import training_loop as tl
    from sid_lsg_amd.unet import CONFIGS, HipUNet2DCondition
    g = np.load(os.path.join(golden_dir, f'loop_{name}.npz'))
    cfg, pt = str(g['cfg']), str(g['prediction_type'])
    cd = F32 if mode == 'fp32' else BF16
    pdir = tmp_path / 'prompts'
    pdir.mkdir()
    (pdir / 'aesthetics_6_plus.txt').write_text('\n'.join(str(p) for p in g['prompts']) + '\n')
    run = tmp_path / 'run'
    run.mkdir()

    def factory(**kw):
        ref, vae, _, te, tok = fixtures.factory(cfg)
        assert abs(fixtures.checksum(ref)[1] - float(g['weight_checksum'][1])) <= 1e-9 * float(g['weight_checksum'][1])
        unet = HipUNet2DCondition(CONFIGS[cfg], compute_dtype=cd)
        unet.prediction_type = pt
        unet.materialize(dev, source=ref.state_dict())
        return unet, vae, _sched(pt).to(dev), te.to(dev), tok
    losses = []
    saved = tl.load_sd15
    try:
        tl.load_sd15 = factory
        tl.training_loop(on_iteration=lambda it, lf, lg: losses.extend([lf, lg]), **_loop_kwargs(g, run, pdir, dev, mode))
    finally:
        tl.load_sd15 = saved
    got, ref = np.array(losses), g['loss_values']
    assert got.shape == ref.shape
    rel_f = np.abs(got[0::2] - ref[0::2]) / np.abs(ref[0::2])
    print(f'loop_{name} {mode}: product {got} reference {ref} fake-loss rel {rel_f}')
    # The generator loss is a small signed sum of large terms (G = psi = phi at the start): its error is also stated on the scale of
    # the run's fake-score loss (same units).  The v golden's generator losses are 0.17 ... 3.5 against fake-score losses up to 500, and
    # its last fake-score loss (7.4) is 50x below the others, so a per-iteration scale would magnify the same absolute error 50x there.
    scale = np.abs(ref[0::2]).max()
    err_g = np.abs(got[1::2] - ref[1::2])
    rel_g = err_g / np.abs(ref[1::2])
    print(f'   G-loss rel {rel_g} err / scale {err_g / scale}')
    if mode == 'fp32':
        assert rel_f.max() < 1e-3
        assert np.all((rel_g < 1e-3) | (err_g / scale < 1e-5)), rel_g
    else:
        assert rel_f[0] < 2e-3 and rel_f.max() < 6e-3
        assert (err_g / scale).max() < 2e-2


# ---- the step's fast paths at N = 2 ---------------------------------------------------------------------------------------------
def _step_run(dev, *, graphed=False, iters=2, rounds=1, early=True, reducer=None, n=2):
    from sid_lsg_amd.optim import FusedAdamEMA
    from sid_lsg_amd.sid_step import SiDStep
    from sid_lsg_amd.unet import CONFIGS, HipUNet2DCondition
    cfg_name, lat, b, lr = 'tiny40', 16, 2, 2e-5
    cfg = CONFIGS[cfg_name]
    phi = HipUNet2DCondition(cfg).materialize(dev, seed=1).requires_grad_(False)
    psi = HipUNet2DCondition(cfg).materialize(dev, seed=2)
    G, G_ema = phi.clone_network(), phi.clone_network(with_grad_buffers=False)
    step = SiDStep(G, psi, phi, G_ema, _sched('epsilon').to(dev), FusedAdamEMA(psi.parameters(), lr=lr, betas=(0.0, 0.999)),
                   FusedAdamEMA(G.parameters(), lr=lr, betas=(0.0, 0.999)), alpha=1.0, cfg_train_fake=1.5, cfg_eval_fake=1.5,
                   cfg_eval_real=2.0, batch_gpu_total=rounds * b, init_timestep=625, reducer=reducer, num_steps=n)
    step.early_gfwd = early
    gen = torch.Generator().manual_seed(3)
    losses = []
    for it in range(iters):
        inputs = {ph: [dict(z=torch.randn(b, 4, lat, lat, generator=gen).to(dev), noise=torch.randn(b, 4, lat, lat, generator=gen).to(dev),
                            t=torch.randint(20, 980, (b,), generator=gen).to(dev),
                            cond=torch.randn(b, cfg.text_len, cfg.cross_attention_dim, generator=gen).to(dev).to(BF16),
                            uncond=torch.randn(b, cfg.text_len, cfg.cross_attention_dim, generator=gen).to(dev).to(BF16),
                            eps_next=torch.randn(n - 1, b, 4, lat, lat, generator=gen).to(dev)) for _ in range(rounds)]
                  for ph in ('A', 'B')}
        lf, lg = (step.iteration_graphed if graphed else step.iteration)(inputs, ema_beta=0.5 + 0.1 * it)
        losses += [float(lf), float(lg)]
    torch.cuda.synchronize()
    return dict(losses=np.array(losses), G=G.flat_params.clone(), psi=psi.flat_params.clone(), ema=G_ema.flat_params.clone(),
                ngraphs=len(step._graphs)), lr


def _assert_same_run(a, g, lr, iters, loss_tol):
    rel = np.abs(a['losses'] - g['losses']) / np.abs(a['losses'])
    print(f'losses {a["losses"]} vs {g["losses"]}: rel {rel}')
    assert rel.max() < loss_tol
    for k in ('G', 'psi', 'ema'):
        d = (a[k] - g[k]).abs()
        same = float((d < 1e-9).float().mean())
        print(f'{k}: {same:.5f} of the weights bit-equal, max difference {float(d.max()):.2e} (lr {lr})')
        # an Adam(beta1 = 0) step is +-lr: only weights with a ~0 gradient may flip (fp32 atomics / split-K order)
        assert float(d.max()) <= 2.01 * lr * iters and same > 0.98


def test_multistep_step_early_forward_and_grad_assign_change_nothing(dev, monkeypatch):
    """SIDLSG_EARLY_GFWD 0 / 1 and SIDLSG_GRAD_ASSIGN 0 / 1 at N = 2: the generator's N weight-gradient launches per layer (first one
    overwrites, the rest accumulate) give the same step; also with two accumulation rounds (grouped wgrad queue flushed per dW)."""
    runs = {}
    for assign in ('1', '0'):
        monkeypatch.setenv('SIDLSG_GRAD_ASSIGN', assign)
        for early in (True, False):
            runs[(assign, early)], lr = _step_run(dev, early=early)
    base = runs[('1', True)]
    for key, r in runs.items():
        if key != ('1', True):
            _assert_same_run(base, r, lr, 2, 2e-3)
    monkeypatch.setenv('SIDLSG_GRAD_ASSIGN', '1')
    a, _ = _step_run(dev, rounds=2)
    monkeypatch.setenv('SIDLSG_GRAD_ASSIGN', '0')
    b, _ = _step_run(dev, rounds=2)
    _assert_same_run(a, b, lr, 2, 2e-3)


def test_multistep_graphed_iteration_equals_eager(dev):
    a, lr = _step_run(dev, iters=3)
    g, _ = _step_run(dev, graphed=True, iters=3)
    assert g['ngraphs'] == 1
    _assert_same_run(a, g, lr, 3, 2e-4)


@pytest.mark.parametrize('n,rounds', [(2, 1), (4, 2)])
def test_multistep_deterministic_runs_are_bit_equal(dev, n, rounds):
    """SIDLSG deterministic mode at N = 2 and at N = 4 with two accumulation rounds (the later gradient adds land on non-zero
    values): two runs bit-equal."""
    from sid_lsg_amd import ops
    ops.set_deterministic(True)
    try:
        a, _ = _step_run(dev, n=n, rounds=rounds)
        b, _ = _step_run(dev, n=n, rounds=rounds)
    finally:
        ops.set_deterministic(None)
    assert np.array_equal(a['losses'], b['losses'])
    for k in ('G', 'psi', 'ema'):
        assert torch.equal(a[k], b[k]), k


def test_a_parameter_reached_twice_flushes_its_queued_reduction(dev):
    """Deferred dgamma / dbeta reductions (csrc/norm.hip): a LayerNorm applied three times with the same parameters in one graph.
    Each later use launches what is queued before queuing its own reduction, so at the end of the backward one job is pending, not
    three, and the three sums reach dgamma / dbeta in stream order (one batched launch would let their atomics commit in any order).
    The gradients equal those of the same graph with every reduction launched at once (SIDLSG_DEFER_REDUCE=0 semantics: one launch
    per layer, in order) bit for bit in deterministic mode."""
    from sid_lsg_amd import ops
    from sid_lsg_amd._lib import lib
    if not ops._DEFER:
        pytest.skip('deferred reductions are switched off (SIDLSG_DEFER_REDUCE=0)')
    C, rows = 320, 96
    g = torch.Generator().manual_seed(2)
    x0 = torch.randn(rows, C, generator=g).to(dev).to(BF16)
    w = torch.randn(rows, C, generator=g).to(dev)
    gam0 = (1 + 0.1 * torch.randn(C, generator=g)).to(dev)
    bet0 = (0.1 * torch.randn(C, generator=g)).to(dev)
    seen = []

    class Probe(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return x.view_as(x)

        @staticmethod
        def backward(ctx, gr):          # runs after the three LayerNorm backward nodes, before the end-of-backward flush
            seen.append(lib.sidlsg_pending_reductions.raw(torch.cuda.current_stream().cuda_stream))
            return gr

    def run(defer):
        gamma, beta = torch.nn.Parameter(gam0.clone()), torch.nn.Parameter(bet0.clone())
        gamma.grad, beta.grad = torch.full_like(gam0, 0.25), torch.full_like(bet0, -0.5)     # later adds land on a value
        saved = ops._DEFER
        ops._DEFER = defer
        try:
            y = Probe.apply(x0.clone().requires_grad_(True))
            for _ in range(3):
                y = ops.layer_norm(y, gamma, beta)
            (y.float() * w).sum().backward()
        finally:
            ops._DEFER = saved
        torch.cuda.synchronize()
        return gamma.grad.clone(), beta.grad.clone()

    ops.set_deterministic(True)
    try:
        dg, db = run(True)
        assert seen == [1], seen
        dg0, db0 = run(False)
    finally:
        ops.set_deterministic(None)
    assert torch.equal(dg, dg0) and torch.equal(db, db0)


def test_multistep_exchange_on_rccl_world1_with_segment_overlap(dev):
    """Gradient exchange forced on RCCL at world 1 with the segment-wise overlap (markers only on G's step-0 forward; early generator
    forward on and off) against the same step without exchange: equal within atomics noise.  In a child process (its own process
    group: tests/mp_multistep_worker.py)."""
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT=str(_free_port()))
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'mp_multistep_worker.py'), 'rccl1'], env=env, capture_output=True,
                       text=True, timeout=600)
    print(r.stdout[-4000:], r.stderr[-3000:])
    assert r.returncode == 0 and 'rccl1 ok' in r.stdout


def test_multistep_refuses_several_wgrad_streams(dev):
    """SIDLSG_WGRAD_STREAMS > 1 cannot keep a layer's N weight-gradient launches ordered: refused for a grad-enabled N-step forward."""
    code = ('import torch, sys; sys.path.insert(0, %r)\n'
            'from sid_lsg_amd.sd_util import hip_generate_steps\n'
            'from sid_lsg_amd.scheduler import DDPMScheduler\n'
            'from sid_lsg_amd.unet import CONFIGS, HipUNet2DCondition\n'
            'dev = torch.device("cuda:0"); cfg = CONFIGS["tiny"]\n'
            'G = HipUNet2DCondition(cfg).materialize(dev, seed=1).train().requires_grad_(True)\n'
            'z = torch.randn(1, 4, 8, 8, device=dev); e = torch.randn(1, 1, 4, 8, 8, device=dev)\n'
            'ctx = torch.randn(1, cfg.text_len, cfg.cross_attention_dim, device=dev).to(torch.bfloat16)\n'
            't = torch.full((1,), 625, dtype=torch.long, device=dev)\n'
            'try:\n'
            '    hip_generate_steps(G, z, e, ctx, t, DDPMScheduler().to(dev))\n'
            'except RuntimeError as ex:\n'
            '    print("refused:", ex); sys.exit(0)\n'
            'sys.exit(3)\n') % ROOT
    env = dict(os.environ, SIDLSG_WGRAD_STREAMS='2')
    r = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0 and 'SIDLSG_WGRAD_STREAMS' in r.stdout


def _free_port():
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        return sk.getsockname()[1]


def test_multistep_mode2_ddp_wrapper_exchanges_once_per_backward(dev, tmp_path):
    """INTEGRATION.md mode 2 at N = 2: the generator wrapped in DistributedDataParallel and handed to the N-step sampler, 2 gloo ranks
    sharing the GPU.  Only the step-0 forward places the exchange: one all-reduce per backward, none under no_sync, and the flat
    gradient buffer ends as the mean over ranks of the local gradients (tests/mp_multistep_worker.py ddp2)."""
    out = str(tmp_path / 'ddp2')
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
           '--master-port', str(_free_port()), os.path.join(ROOT, 'tests', 'mp_multistep_worker.py'), 'ddp2', out]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    for rank in (0, 1):
        d = np.load(f'{out}.rank{rank}.npz')
        print(f"rank {rank}: exchanges no_sync {int(d['n_nosync'])} sync {int(d['n_sync'])}, error {float(d['err']):.2e}, "
              f"local-vs-mean {float(d['local_vs_mean']):.2e}")
        assert int(d['n_nosync']) == 0 and int(d['n_sync']) == 1
        assert float(d['local_vs_mean']) > 1e-3, 'the ranks must have different local gradients for this test to mean anything'
        assert float(d['err']) < 2e-5


def test_cli_trains_a_two_step_generator_and_generates_from_it(tmp_path):
    """sid_train.py --num_steps 2 runs a couple of ticks and writes a snapshot; generate_onestep.py loads it."""
    from click.testing import CliRunner
    import generate_onestep
    import sid_train
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    (tmp_path / 'aesthetics_6_plus.txt').write_text('\n'.join(f'prompt number {i}' for i in range(40)) + '\n')
    runs = tmp_path / 'runs'
    res = CliRunner().invoke(sid_train.main, [
        '--outdir', str(runs), '--data_prompt_text', str(tmp_path), '--sd_model', 'random:tiny', '--seed', '1', '--batch', '4',
        '--batch-gpu', '2', '--duration', '0.00002', '--ema', '0.00001', '--tick', '1', '--snap', '1', '--dump', '1',
        '--cfg_train_fake', '1.5', '--cfg_eval_fake', '1.5', '--cfg_eval_real', '1.5', '--resolution', '128', '--num_steps', '2'],
        catch_exceptions=False)
    assert res.exit_code == 0, res.output
    run_dir = glob.glob(str(runs / '00000-*'))[0]
    assert len([ln for ln in open(os.path.join(run_dir, 'stats_1.000000.jsonl'))]) >= 2       # a couple of ticks
    snaps = sorted(glob.glob(os.path.join(run_dir, 'network-snapshot-*.pkl')))
    assert snaps
    out = tmp_path / 'img'
    res = CliRunner().invoke(generate_onestep.main, [
        '--network', snaps[-1], '--outdir', str(out), '--seeds', '0-1', '--batch', '2',
        '--text_prompts', str(tmp_path / 'aesthetics_6_plus.txt'), '--repo_id', 'random:tiny'], catch_exceptions=False)
    assert res.exit_code == 0, res.output
    assert sorted(os.path.basename(f) for f in glob.glob(str(out / '*.png'))) == ['000000.png', '000001.png']
