"""v-prediction (SD 2.x 768-v) teachers on the GPU: the mode-2 CFG/x0 kernels and the v fake-score loss against float64
torch, the epsilon kernels against a build of their previous source, the product loop against the unmodified reference loop
under a v scheduler (tests/golden/loop_v_*.npz), one full-size SD2.1-v iteration against the stored CPU oracle, the step's
consistency switches in v mode, and generation from a v snapshot."""
import copy
import ctypes
import glob
import os
import pickle
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
V = 'v_prediction'


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from sid_lsg_amd._lib import lib
    lib.load()
    return torch.device('cuda:0')


def _coefs(t):
    from sid_lsg_amd.scheduler import DDPMScheduler
    ab = torch.cumprod(1 - torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float64) ** 2, 0)
    s = DDPMScheduler(prediction_type=V)
    a = s.alphas_cumprod[t].double()
    return s, a.sqrt(), (1 - a).sqrt(), ab


# ---- kernels ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dup', [1, 2])
@pytest.mark.parametrize('kappa', [1.0, 2.5])
@pytest.mark.parametrize('act', [BF16, F32])
def test_cfg_x0_v_mode_forward_backward(dev, dup, kappa, act):
    from sid_lsg_amd import ops
    B, C, H, W = 3, 4, 8, 12
    g = torch.Generator().manual_seed(1)
    t = torch.tensor([20, 625, 979])
    sched, s0, s1, _ = _coefs(t)
    eps = torch.zeros(dup * B, H * W, 8)
    eps[..., :C] = torch.randn(dup * B, H * W, C, generator=g)
    xt = torch.randn(B, C, H, W, generator=g)
    gout = torch.randn(B, C, H, W, generator=g)
    d_s0, d_s1 = sched.to(dev).coefficients(t.to(dev))
    e_d = eps.to(dev).requires_grad_()
    x_d = xt.to(dev).requires_grad_()
    out = ops.cfg_x0(e_d, x_d, d_s0, d_s1, kappa, True, act, prediction_type=V)
    out.backward(gout.to(dev))
    # float64 closed form
    e64 = eps.double()[..., :C].reshape(dup * B, H, W, C).permute(0, 3, 1, 2)
    e = e64[:B] + kappa * (e64[B:] - e64[:B]) if dup == 2 else e64
    S0, S1 = s0.view(-1, 1, 1, 1), s1.view(-1, 1, 1, 1)
    ref = S0 * xt.double() - S1 * e
    assert float((out.detach().cpu().double() - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
    ge = -S1 * gout.double()                                      # d out / d e
    dxt_ref = S0 * gout.double()
    assert float((x_d.grad.cpu().double() - dxt_ref).abs().max()) <= 1e-6 * float(dxt_ref.abs().max())
    parts = [(1 - kappa) * ge, kappa * ge] if dup == 2 else [ge]
    de_ref = torch.zeros(dup * B, H * W, 8, dtype=torch.float64)
    for i, p in enumerate(parts):
        de_ref[i * B:(i + 1) * B, :, :C] = p.permute(0, 2, 3, 1).reshape(B, H * W, C)
    got = e_d.grad.cpu().double()
    tol = 4e-3 if act == BF16 else 1e-6                           # bf16: one rounding of the gradient handed to the network
    assert float((got - de_ref).abs().max()) <= tol * float(de_ref.abs().max())
    assert float(got[..., C:].abs().max()) == 0.0                 # padding channels stay zero
    # raw output (predict_x0 False) is the mode-0 kernel whatever the parameterisation
    raw = ops.cfg_x0(eps.to(dev), xt.to(dev), d_s0, d_s1, kappa, False, act, prediction_type=V)
    assert float((raw.cpu().double() - e).abs().max()) <= 1e-6 * float(e.abs().max())


def test_cfg_x0_rejects_an_unknown_mode(dev):
    from sid_lsg_amd._lib import lib
    x = torch.zeros(1, 4, 2, 2, device=dev)
    eps = torch.zeros(1, 4, 8, device=dev)
    s = torch.ones(1, device=dev)
    with pytest.raises(RuntimeError):
        lib.sidlsg_cfg_x0(eps.data_ptr(), x.data_ptr(), s.data_ptr(), s.data_ptr(), x.data_ptr(), 1, 4, 4, 8, 1, 1.0, 3,
                          torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize('nan_in', [None, 'o', 'images'])
def test_fake_loss_v_value_and_gradient(dev, nan_in):
    from sid_lsg_amd import ops
    B, C, H, W = 4, 4, 16, 16
    g = torch.Generator().manual_seed(2)
    t = torch.tensor([21, 300, 625, 970])
    sched, s0, s1, ab = _coefs(t)
    o, images, noise = (torch.randn(B, C, H, W, generator=g) for _ in range(3))
    if nan_in == 'o':
        o[1, 2, 3, 4] = float('nan')
    elif nan_in == 'images':
        images[2, 0, 5, 6] = float('nan')
    scale = 0.25
    d_s0, d_s1 = sched.to(dev).coefficients(t.to(dev))
    w = sched.snr_weights(t.to(dev))
    od = o.to(dev).requires_grad_()
    loss = ops.sid_fake_score_loss_v(od, images.to(dev), noise.to(dev), d_s0, d_s1, w, scale)
    loss.backward()
    S0, S1 = s0.view(-1, 1, 1, 1), s1.view(-1, 1, 1, 1)
    v = S0 * noise.double() - S1 * images.double()
    a = ab[t]
    w64 = (a / (1 - a)) / (a / (1 - a) + 1)
    keep = ~(torch.isnan(o).flatten(1).any(1) | torch.isnan(v).flatten(1).any(1))
    assert int(keep.sum()) == (B if nan_in is None else B - 1)
    d = o.double() - v
    ref = float(((d ** 2).sum((1, 2, 3)) * w64)[keep].sum() * scale)
    assert abs(float(loss.detach()) - ref) <= 1e-5 * abs(ref)
    gref = 2 * scale * w64.view(-1, 1, 1, 1) * d
    gref[~keep] = 0
    got = od.grad.cpu().double()
    assert torch.isfinite(got).all()
    assert float((got - gref).abs().max()) <= 1e-5 * float(gref.abs().max())
    assert float(got[~keep].abs().max() if (~keep).any() else 0.0) == 0.0


# the epsilon kernels as they were before the mode argument existed (formulas of the previous elementwise.hip)
_EPS_COPY = r'''
#include "common.h"
__global__ void old_cfg_x0(const float* eps, const float* xt, const float* s0, const float* s1, float* out, int B, int C, int HW,
                           int Ce, int dup, float kappa, int predict_x0) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= B * HW) return;
    const int b = idx / HW, p = idx - b * HW;
    for (int c = 0; c < C; c++) {
        float e = eps[((size_t)b * HW + p) * Ce + c];
        if (dup == 2) { const float cnd = eps[((size_t)(B + b) * HW + p) * Ce + c]; e = e + kappa * (cnd - e); }
        const size_t i = ((size_t)b * C + c) * HW + p;
        out[i] = predict_x0 ? (xt[i] - s1[b] * e) / s0[b] : e;
    }
}
template <typename T>
__global__ void old_cfg_x0_bwd(const float* g, const float* s0, const float* s1, T* deps, float* dxt, int B, int C, int HW, int Cp,
                               int dup, float kappa, int predict_x0) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= B * HW) return;
    const int b = idx / HW, p = idx - b * HW;
    float du[8] = {0, 0, 0, 0, 0, 0, 0, 0}, dc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int c = 0; c < C; c++) {
        const size_t i = ((size_t)b * C + c) * HW + p;
        const float go = g[i];
        const float ge = predict_x0 ? -go * s1[b] / s0[b] : go;
        if (dxt) dxt[i] = predict_x0 ? go / s0[b] : 0.f;
        if (dup == 2) { du[c] = (1.f - kappa) * ge; dc[c] = kappa * ge; }
        else du[c] = ge;
    }
    T* d0 = deps + ((size_t)b * HW + p) * Cp;
    stv8<T>(d0, du);
    for (int c = 8; c < Cp; c += 8) zerov8<T>(d0 + c);
    if (dup == 2) {
        T* d1 = deps + ((size_t)(B + b) * HW + p) * Cp;
        stv8<T>(d1, dc);
        for (int c = 8; c < Cp; c += 8) zerov8<T>(d1 + c);
    }
}
extern "C" int old_fwd(const float* eps, const float* xt, const float* s0, const float* s1, float* out, int B, int C, int HW, int Ce,
                       int dup, float kappa, int px0, void* stream) {
    hipLaunchKernelGGL(old_cfg_x0, dim3((B * HW + 255) / 256), dim3(256), 0, (hipStream_t)stream, eps, xt, s0, s1, out, B, C, HW, Ce, dup, kappa, px0);
    return (int)hipGetLastError();
}
extern "C" int old_bwd(const float* g, const float* s0, const float* s1, void* deps, float* dxt, int B, int C, int HW, int Cp, int dup,
                       float kappa, int px0, int f32, void* stream) {
    if (f32) hipLaunchKernelGGL(old_cfg_x0_bwd<float>, dim3((B * HW + 255) / 256), dim3(256), 0, (hipStream_t)stream, g, s0, s1, (float*)deps, dxt, B, C, HW, Cp, dup, kappa, px0);
    else hipLaunchKernelGGL(old_cfg_x0_bwd<bf16>, dim3((B * HW + 255) / 256), dim3(256), 0, (hipStream_t)stream, g, s0, s1, (bf16*)deps, dxt, B, C, HW, Cp, dup, kappa, px0);
    return (int)hipGetLastError();
}
'''


@pytest.fixture(scope='module')
def eps_copy(tmp_path_factory):
    from sid_lsg_amd.csrc import build
    d = tmp_path_factory.mktemp('eps_copy')
    src, so = d / 'eps_copy.hip', d / 'libeps_copy.so'
    src.write_text(_EPS_COPY)
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    subprocess.check_call([hipcc] + build.FLAGS + ['-shared', '-I', build.HERE, str(src), '-o', str(so)])
    lib = ctypes.CDLL(str(so))
    P, I, Fl = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    lib.old_fwd.argtypes = [P, P, P, P, P, I, I, I, I, I, Fl, I, P]
    lib.old_bwd.argtypes = [P, P, P, P, P, I, I, I, I, I, Fl, I, I, P]
    return lib


@pytest.mark.parametrize('dup', [1, 2])
@pytest.mark.parametrize('px0', [0, 1])
def test_eps_modes_are_bit_equal_to_the_previous_kernels(dev, eps_copy, dup, px0):
    """Modes 0 / 1 are the former predict_x0 = 0 / 1: bit for bit, forward and both backward variants."""
    from sid_lsg_amd import ops
    from sid_lsg_amd.scheduler import DDPMScheduler
    B, C, HW = 2, 4, 96
    g = torch.Generator().manual_seed(3)
    eps = torch.zeros(dup * B, HW, 8)
    eps[..., :C] = torch.randn(dup * B, HW, C, generator=g)
    eps = eps.to(dev)
    xt = torch.randn(B, C, 8, 12, generator=g).to(dev)
    gout = torch.randn(B, C, 8, 12, generator=g).to(dev)
    s0, s1 = DDPMScheduler().to(dev).coefficients(torch.tensor([37, 811], device=dev))
    stream = torch.cuda.current_stream().cuda_stream
    kappa = 1.7
    ref = torch.empty_like(xt)
    assert eps_copy.old_fwd(eps.data_ptr(), xt.data_ptr(), s0.data_ptr(), s1.data_ptr(), ref.data_ptr(), B, C, HW, 8, dup, kappa, px0, stream) == 0
    e_d, x_d = eps.clone().requires_grad_(), xt.clone().requires_grad_()
    out = ops.cfg_x0(e_d, x_d, s0, s1, kappa, bool(px0), BF16)
    assert torch.equal(out.detach(), ref)
    out.backward(gout)
    for act in (BF16, F32):
        deps = torch.empty(dup * B, HW, 8, device=dev, dtype=act)
        dxt = torch.empty_like(xt)
        assert eps_copy.old_bwd(gout.data_ptr(), s0.data_ptr(), s1.data_ptr(), deps.data_ptr(), dxt.data_ptr(), B, C, HW, 8, dup, kappa,
                                px0, int(act == F32), stream) == 0
        if act == BF16:
            assert torch.equal(e_d.grad, deps.float()) and torch.equal(x_d.grad, dxt)     # (autograd hands eps an fp32 copy of the bf16 gradient)
        else:
            e2, x2 = eps.clone().requires_grad_(), xt.clone().requires_grad_()
            ops.cfg_x0(e2, x2, s0, s1, kappa, bool(px0), F32).backward(gout)
            assert torch.equal(e2.grad, deps) and torch.equal(x2.grad, dxt)


# ---- glue against the reference's sid_sd_sampler / sid_sd_denoise under the v scheduler -------------------------------------
def test_v_glue_matches_reference_golden(dev, golden_dir):
    from oracle import fixtures
    from sid_lsg_amd.scheduler import DDPMScheduler
    from sid_lsg_amd.sd_util import sid_sd_denoise, sid_sd_sampler
    from sid_lsg_amd.unet import CONFIGS, HipUNet2DCondition
    g = np.load(os.path.join(golden_dir, 'glue_v_tiny.npz'))
    ref1, _, _, te, tok = fixtures.factory('tiny')
    ref2 = fixtures.make_unet('tiny', seed=99)
    hip1 = HipUNet2DCondition(CONFIGS['tiny'], compute_dtype=F32).materialize(dev, source=ref1.state_dict())
    hip2 = HipUNet2DCondition(CONFIGS['tiny'], compute_dtype=F32).materialize(dev, source=ref2.state_dict())
    sched = DDPMScheduler(prediction_type=V).to(dev)
    with pytest.raises(ValueError):          # an epsilon network under a v scheduler
        sid_sd_sampler(hip1, torch.zeros(1, 4, 8, 8, device=dev), ['x'], torch.full((1,), 625, device=dev), sched, te.to(dev), tok, 64)
    hip1.prediction_type = hip2.prediction_type = V
    te = te.to(dev)
    for b in (1, 2):
        z, noise = torch.from_numpy(g[f'b{b}_z']).to(dev), torch.from_numpy(g[f'b{b}_noise']).to(dev)
        t = torch.from_numpy(g[f'b{b}_t']).to(dev)
        prompts = [str(p) for p in g[f'b{b}_prompts']]
        with torch.no_grad():
            xhat = sid_sd_sampler(hip1, z, prompts, torch.full((b,), 625, dtype=torch.long, device=dev), sched, te, tok, 64, dtype=F32)
        ref = torch.from_numpy(g[f'b{b}_xhat'])
        e = float((xhat.cpu() - ref).abs().max() / ref.abs().max())
        assert e < 1e-4, f'sampler b{b}: {e}'
        xh = ref.to(dev)
        for kappa in (1.0, 2.0):
            for px0 in (True, False):
                with torch.no_grad():
                    y = sid_sd_denoise(hip2, xh, noise, prompts, t, sched, te, tok, 64, dtype=F32, predict_x0=px0, guidance_scale=kappa)
                r = torch.from_numpy(g[f'b{b}_k{kappa}_x0{int(px0)}'])
                e = float((y.cpu() - r).abs().max() / r.abs().max())
                print(f'v denoise b{b} kappa {kappa} x0 {px0}: {e:.2e}')
                assert e < 1e-4, f'denoise b{b} k{kappa} x0{px0}: {e}'


# ---- the product loop against the unmodified reference loop under a v scheduler ----------------------------------------------
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
                cfg_eval_real=kappa[2], resolution=int(g['kw_resolution']), enable_xformers=False, rng_device='cpu')


@pytest.mark.parametrize('mode', ['fp32', 'bf16'])
@pytest.mark.parametrize('name', ['k15_a1', 'k1_a12'])
def test_product_loop_matches_reference_v_golden(dev, golden_dir, tmp_path, name, mode):
    """training_loop(**c) with a v-prediction teacher (scheduler and networks) against the unmodified reference training_loop
    under the v scheduler (tools/make_vpred_goldens.py).  The epsilon path computes other losses from iteration 0 on."""
    from oracle import fixtures
    from sid_lsg_amd import training_loop as tl
    from sid_lsg_amd.scheduler import DDPMScheduler
    from sid_lsg_amd.unet import CONFIGS, HipUNet2DCondition
    g = np.load(os.path.join(golden_dir, f'loop_v_{name}.npz'))
    cfg = str(g['cfg'])
    cd = BF16 if mode == 'bf16' else F32
    pdir = tmp_path / 'prompts'
    pdir.mkdir()
    (pdir / 'aesthetics_6_plus.txt').write_text('\n'.join(str(p) for p in g['prompts']) + '\n')
    run = tmp_path / 'run'
    run.mkdir()

    def factory(**kw):
        ref, vae, _, te, tok = fixtures.factory(cfg)
        assert abs(fixtures.checksum(ref)[1] - float(g['weight_checksum'][1])) <= 1e-9 * float(g['weight_checksum'][1])
        unet = HipUNet2DCondition(CONFIGS[cfg], compute_dtype=cd).materialize(dev, source=ref.state_dict())
        unet.prediction_type = V
        return unet, vae, DDPMScheduler(prediction_type=V).to(dev), te.to(dev), tok
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
    abs_g = np.abs(got[1::2] - ref[1::2]) / np.abs(ref[0::2])         # generator loss error on the loss scale (as the epsilon loop tests)
    print(f'loop_v_{name} [{mode}]: product {got} reference {ref} fake-loss rel {rel_f} G-loss err / scale {abs_g}')
    if mode == 'fp32':
        rel_g = np.abs(got[1::2] - ref[1::2]) / np.abs(ref[1::2])
        assert rel_f.max() < 1e-3 and rel_g.max() < 1e-3, f'fp32: {rel_f} {rel_g}'
    else:           # the bounds of tests/test_gpu_unet.py::test_product_loop_matches_reference_golden
        assert rel_f[0] < 2e-3 and rel_f.max() < 6e-3
        assert abs_g.max() < 2e-2


# ---- one full-size SD2.1-v iteration against the stored CPU oracle ----------------------------------------------------------
@pytest.mark.parametrize('cd', [F32, BF16])
def test_full_size_sd21_v_iteration_matches_stored_oracle(dev, golden_dir, cd):
    from oracle import fixtures, sid_ref
    from sid_lsg_amd.optim import FusedAdamEMA
    from sid_lsg_amd.scheduler import DDPMScheduler
    from sid_lsg_amd.sid_step import SiDStep
    from sid_lsg_amd.unet import CONFIGS, HipUNet2DCondition
    fx = np.load(os.path.join(golden_dir, 'fullsize_sd21v_k2_512.npz'))
    cfg_name, lat, b, kappa, lr = 'sd21-base', 64, 1, 2.0, fixtures.FULLSIZE_LR
    torch.set_num_threads(min(16, os.cpu_count() or 8))
    try:
        phi_r = fixtures.make_unet_cached(cfg_name)
        psi_r = fixtures.make_unet_cached(cfg_name, seed=77)
        cks = np.array(fixtures.checksum(phi_r) + fixtures.checksum(psi_r))
    finally:
        torch.set_num_threads(min(8, os.cpu_count() or 8))
    assert np.all(np.abs(cks - fx['weight_checksum']) <= 1e-9 * np.abs(fx['weight_checksum']))

    def hipnet(r):
        n = HipUNet2DCondition(CONFIGS[cfg_name], compute_dtype=cd).materialize(dev, source=r.state_dict())
        n.prediction_type = V
        return n
    phi, psi, G, G_ema = hipnet(phi_r), hipnet(psi_r), hipnet(phi_r), hipnet(phi_r)
    del phi_r
    init = {key: {n: p.detach().clone() for n, p in net.named_parameters()} for key, net in (('psi', psi), ('G', G))}
    step = SiDStep(G, psi, phi, G_ema, DDPMScheduler(prediction_type=V).to(dev),
                   FusedAdamEMA(psi.parameters(), lr=lr, betas=(0.0, 0.999), eps=1e-8),
                   FusedAdamEMA(G.parameters(), lr=lr, betas=(0.0, 0.999), eps=1e-8), alpha=1.0, cfg_train_fake=kappa,
                   cfg_eval_fake=kappa, cfg_eval_real=kappa, batch_gpu_total=b, init_timestep=625)
    inputs = fixtures.iteration_inputs(cfg_name, lat, b, 1, torch.Generator().manual_seed(fixtures.FULLSIZE_SEED))
    dinp = {ph: [{k: (v.to(dev).to(cd).contiguous() if k in ('cond', 'uncond') else v.to(dev)) for k, v in r.items()} for r in inputs[ph]]
            for ph in inputs}
    lf, lg = step.iteration(dinp, ema_beta=sid_ref.ema_beta_ref(b, 0, 50, 0.05))
    rf = abs(float(lf) - float(fx['loss_fake'])) / abs(float(fx['loss_fake']))
    rg = abs(float(lg) - float(fx['loss_G'])) / abs(float(fx['loss_G']))
    print(f'SD2.1-v 512 [{cd}]: loss_fake {float(lf):.6f} vs {float(fx["loss_fake"]):.6f} (rel {rf:.1e}); '
          f'loss_G {float(lg):.6f} vs {float(fx["loss_G"]):.6f} (rel {rg:.1e})')
    if cd == F32:
        assert rf <= 1e-3 and rg <= 1e-3
    else:
        assert rf <= 2e-3 and rg <= 1e-2
    # update directions (every 431st weight) and the EMA weights, as tests/test_gpu_unet.py::_iteration_parity checks them
    for name, key, net in (('fake_score', 'psi', psi), ('G', 'G', G)):
        n_s = int(fx[name + '/n'])
        sign_r = torch.from_numpy(np.unpackbits(fx[name + '/sign'])[:n_s].astype(bool)).to(dev)
        big_r = torch.from_numpy(np.unpackbits(fx[name + '/big'])[:n_s].astype(bool)).to(dev)
        mine, pos, agree, total = dict(net.named_parameters()), 0, 0, 0
        for n, pr in psi_r.named_parameters():
            idx = fixtures.sample_index(pr.numel()).to(dev)
            du = mine[n].detach().flatten()[idx] - init[key][n].flatten()[idx]
            sr, big = sign_r[pos:pos + idx.numel()], big_r[pos:pos + idx.numel()]
            pos += idx.numel()
            agree += int((big & (du != 0) & ((du > 0) == sr)).sum())
            total += int(big.sum())
        assert pos == n_s
        frac = agree / max(total, 1)
        print(f'{name} [{cd}]: update-sign agreement {frac:.4f} over {total} weights')
        assert frac > (0.99 if cd == F32 else 0.96)
    for n, p in G_ema.named_parameters():
        if n in fixtures.FULLSIZE_EMA_NAMES:
            r = torch.from_numpy(fx['ema/' + n])
            e = float((p.detach().cpu() - r).abs().max() / r.abs().max())
            assert e < 2e-3, f'EMA weights {n}: {e}'


# ---- consistency of the step's switches in v mode ---------------------------------------------------------------------------
def _v_step_run(dev, mode, graphed=False, iters=2):
    from sid_lsg_amd.optim import FusedAdamEMA
    from sid_lsg_amd.scheduler import DDPMScheduler
    from sid_lsg_amd.sid_step import SiDStep
    from sid_lsg_amd.unet import CONFIGS, HipUNet2DCondition
    cfg_name, lat, b, lr = 'tiny40', 16, 2, 2e-5
    cfg = CONFIGS[cfg_name]
    phi = HipUNet2DCondition(cfg).materialize(dev, seed=1).requires_grad_(False)
    psi = HipUNet2DCondition(cfg).materialize(dev, seed=2)
    phi.prediction_type = psi.prediction_type = V
    G, G_ema = phi.clone_network(), phi.clone_network(with_grad_buffers=False)
    assert G.prediction_type == V
    step = SiDStep(G, psi, phi, G_ema, DDPMScheduler(prediction_type=V).to(dev), FusedAdamEMA(psi.parameters(), lr=lr, betas=(0.0, 0.999)),
                   FusedAdamEMA(G.parameters(), lr=lr, betas=(0.0, 0.999)), alpha=1.0, cfg_train_fake=1.5, cfg_eval_fake=1.5,
                   cfg_eval_real=2.0, batch_gpu_total=2 * b, init_timestep=625)
    assert step.vpred
    gen = torch.Generator().manual_seed(3)
    losses = []
    for it in range(iters):
        inputs = {ph: [dict(z=torch.randn(b, 4, lat, lat, generator=gen).to(dev), noise=torch.randn(b, 4, lat, lat, generator=gen).to(dev),
                            t=torch.randint(20, 980, (b,), generator=gen).to(dev),
                            cond=torch.randn(b, cfg.text_len, cfg.cross_attention_dim, generator=gen).to(dev).to(BF16),
                            uncond=torch.randn(b, cfg.text_len, cfg.cross_attention_dim, generator=gen).to(dev).to(BF16)) for _ in range(2)]
                  for ph in ('A', 'B')}
        lf, lg = (step.iteration_graphed if graphed else step.iteration)(inputs, ema_beta=0.5 + 0.1 * it)
        losses += [float(lf), float(lg)]
    torch.cuda.synchronize()
    return dict(losses=np.array(losses), G=G.flat_params.clone(), psi=psi.flat_params.clone(), ema=G_ema.flat_params.clone(),
                grouped=step._use_grouped(b), ngraphs=len(step._graphs)), lr


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


def test_v_grouped_frozen_pass_equals_two_stream(dev, monkeypatch):
    """The grouped fake-score + teacher pass (one cfg_x0 per network on the pair's outputs) against the two-stream path in v mode
    (the bounds of tests/test_gpu_grouped.py::test_grouped_frozen_pass_changes_nothing_in_the_step)."""
    out = {}
    for mode in ('0', '1'):
        monkeypatch.setenv('SIDLSG_GROUPED_FROZEN', mode)
        out[mode], lr = _v_step_run(dev, mode)
        assert out[mode]['grouped'] == (mode == '1')
    _assert_same_run(out['0'], out['1'], lr, 2, 2e-3)


def test_v_graphed_iteration_equals_eager(dev):
    a, lr = _v_step_run(dev, 'eager', graphed=False, iters=3)
    g, _ = _v_step_run(dev, 'graph', graphed=True, iters=3)
    assert g['ngraphs'] == 1
    _assert_same_run(a, g, lr, 3, 2e-4)


# ---- generation from a v snapshot ---------------------------------------------------------------------------------------------
def test_generate_768_from_a_v_snapshot(dev, tmp_path):
    from click.testing import CliRunner
    import generate_onestep
    from sid_lsg_amd.unet import CONFIGS, HipUNet2DCondition
    net = HipUNet2DCondition(CONFIGS['tiny']).materialize(dev, seed=4)
    net.prediction_type = V
    snap = tmp_path / 'network-snapshot-v.pkl'
    with open(snap, 'wb') as f:
        pickle.dump(dict(ema=copy.deepcopy(net)), f)
    (tmp_path / 'prompts.txt').write_text('a lighthouse\na red barn\n')
    out = tmp_path / 'img'
    res = CliRunner().invoke(generate_onestep.main, ['--network', str(snap), '--outdir', str(out), '--seeds', '0-1', '--batch', '2',
                                                     '--text_prompts', str(tmp_path / 'prompts.txt'), '--repo_id', 'random:tiny:v',
                                                     '--resolution', '768'], catch_exceptions=False)
    assert res.exit_code == 0, res.output
    files = sorted(glob.glob(str(out / '*.png')))
    assert [os.path.basename(f) for f in files] == ['000000.png', '000001.png']
    import PIL.Image
    assert PIL.Image.open(files[0]).size == (768, 768)
    # the same snapshot with an epsilon --repo_id is refused
    res = CliRunner().invoke(generate_onestep.main, ['--network', str(snap), '--outdir', str(tmp_path / 'img_eps'), '--seeds', '0-1',
                                                     '--text_prompts', str(tmp_path / 'prompts.txt'), '--repo_id', 'random:tiny'])
    assert res.exit_code != 0 and isinstance(res.exception, ValueError), res.output
    assert not glob.glob(str(tmp_path / 'img_eps' / '*.png'))
