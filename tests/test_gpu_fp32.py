"""GPU parity of the fp32-accurate compute mode (csrc/fp32.hip + the _f32 entry-point family).

BASELINE north_star: "outputs match the reference FP32 CPU path ... loss curve matching reference to 1e-3 rel".  The
bf16 production path cannot demonstrate that bound (tests/test_gpu_unet.py states what it does achieve); this mode can,
and the asserts below are that bound or tighter:
  * every fp32 op against an fp64 CPU reference of the same op:            max|err| <= 2e-5 * max|ref|
  * the SD UNet forward / input gradient / parameter gradients vs the fp32 oracle:  1e-4 of max / 1e-3 rel-l2
  * one full SiD-LSG iteration (both phases, Adam, EMA) vs oracle/sid_ref.py: both losses within 1e-3 (observed ~1e-5)
  * the product `training_loop` vs loss curves of the UNMODIFIED reference loop (tests/golden/loop_*.npz): 1e-3
"""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import norm_cases as nc

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
TOL = 2e-5


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from sid_lsg_amd._lib import lib
    lib.load()
    return torch.device('cuda:0')


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def close(got, ref, tol, name=''):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, f'{name}: shape {tuple(got.shape)} vs {tuple(ref.shape)}'
    assert torch.isfinite(got).all(), f'{name}: non-finite output'
    err, scale = (got - ref).abs().max().item(), ref.abs().max().item() + 1e-30
    assert err <= tol * scale, f'{name}: max err {err:.4g} vs scale {scale:.4g} (rel {err / scale:.3g} > {tol})'
    return err / scale


@pytest.mark.parametrize('M,N,K', [(256, 320, 320), (1000, 136, 72), (130, 8, 2880), (77 * 2, 640, 768), (64, 2560, 320)])
def test_gemm_f32(dev, M, N, K):
    from sid_lsg_amd import ops
    a, w = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=K ** -0.5)
    bias, res = rnd(N, seed=3), rnd(M, N, seed=4)
    rpb = M // 2 if M % 2 == 0 else M
    rv = rnd(M // rpb, N, seed=5)
    ref = a.double() @ w.double().t()
    close(ops.gemm(a.to(dev), w.to(dev)), ref, TOL, 'plain')
    full = ref + bias.double() + res.double() + rv.double().repeat_interleave(rpb, 0)
    got = ops.gemm(a.to(dev), w.to(dev), bias=bias.to(dev), res=res.to(dev), rowvec=rv.to(dev), rows_per_batch=rpb)
    assert got.dtype == F32
    close(got, full, TOL, 'epilogue')


CONV_CASES = [(2, 16, 16, 64, 160, 1, 0), (2, 16, 16, 64, 128, 2, 0), (1, 8, 8, 128, 64, 1, 1), (2, 12, 20, 8, 320, 1, 0),
              (2, 8, 8, 320, 8, 1, 0), (3, 9, 7, 72, 40, 2, 0), (1, 16, 16, 640, 160, 1, 1)]


def conv_ref(x, w, stride, ups):
    xn = x.double().permute(0, 3, 1, 2)
    if ups:
        xn = F.interpolate(xn, scale_factor=2.0, mode='nearest')
    cout, k = w.shape
    wn = w.double().view(cout, 3, 3, k // 9).permute(0, 3, 1, 2)
    return F.conv2d(xn, wn, stride=stride, padding=1).permute(0, 2, 3, 1)


@pytest.mark.parametrize('B,H,W,Cin,Cout,stride,ups', CONV_CASES)
def test_conv_autograd_f32(dev, B, H, W, Cin, Cout, stride, ups):
    """forward, dx, dW, db, d(rowvec) of the fp32 conv op against fp64 torch autograd."""
    from sid_lsg_amd import ops
    x, w = rnd(B, H, W, Cin, seed=1), rnd(Cout, 9 * Cin, seed=2, scale=(9 * Cin) ** -0.5)
    bias, rv = rnd(Cout, seed=3), rnd(B, Cout, seed=5)
    xr, wr, br, rvr = (t.double().requires_grad_() for t in (x, w, bias, rv))
    yr = conv_ref(xr, wr, stride, ups) + br + rvr[:, None, None, :]
    dy = rnd(*yr.shape, seed=7)
    yr.backward(dy.double())
    wm = torch.nn.Parameter(w.view(Cout, 3, 3, Cin).permute(0, 3, 1, 2).to(dev))
    wm.grad = torch.zeros(Cout, 3, 3, Cin, device=dev).permute(0, 3, 1, 2)
    bm = torch.nn.Parameter(bias.to(dev))
    bm.grad = torch.zeros_like(bm)
    w32 = w.to(dev)
    w32t = ops.transpose_w(wm.permute(0, 2, 3, 1), Cout, Cin, 9, dtype=F32)
    xd, rvd = x.to(dev).requires_grad_(), rv.to(dev).requires_grad_()
    y = ops.conv3x3_op(xd, wm, bm, w32, w32t, None, rvd, stride, ups, False)
    assert y.dtype == F32
    close(y, yr, TOL, 'fwd')
    y.backward(dy.to(dev))
    close(xd.grad, xr.grad, TOL, 'dx')
    close(wm.grad.permute(0, 2, 3, 1).reshape(Cout, -1), wr.grad, TOL, 'dW')
    close(bm.grad, br.grad, TOL, 'db')
    close(rvd.grad, rvr.grad, TOL, 'd_rowvec')


def test_linear_autograd_f32(dev):
    from sid_lsg_amd import ops
    M, N, K = 520, 320, 640
    x, w, bias, res = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=K ** -0.5), rnd(N, seed=3), rnd(M, N, seed=4)
    xr, wr, br, rr = (t.double().requires_grad_() for t in (x, w, bias, res))
    yr = xr @ wr.t() + br + rr
    dy = rnd(M, N, seed=7)
    yr.backward(dy.double())
    wm = torch.nn.Parameter(w.to(dev)); wm.grad = torch.zeros_like(wm)
    bm = torch.nn.Parameter(bias.to(dev)); bm.grad = torch.zeros_like(bm)
    xd, rd = x.to(dev).requires_grad_(), res.to(dev).requires_grad_()
    y = ops.linear(xd, wm, bm, w.to(dev), ops.transpose_w(wm, N, K, 1, dtype=F32), res=rd)
    close(y, yr, TOL, 'fwd')
    y.backward(dy.to(dev))
    close(xd.grad, xr.grad, TOL, 'dx')
    close(rd.grad, rr.grad, TOL, 'dres')
    close(wm.grad, wr.grad, TOL, 'dW')
    close(bm.grad, br.grad, TOL, 'db')


@pytest.mark.parametrize('B,HW,C,G,silu', [(2, 64, 32, 8, 1), (3, 1024, 320, 32, 1), (2, 256, 1920, 32, 1), (2, 100, 80, 8, 0)])
def test_groupnorm_f32(dev, B, HW, C, G, silu):
    from sid_lsg_amd import ops
    x = rnd(B, HW, C, seed=1) * 1.5 + 0.3
    gam, bet = rnd(C, seed=2) * 0.5 + 1, rnd(C, seed=3) * 0.3
    xr, gr, br = (t.double().requires_grad_() for t in (x, gam, bet))
    yr = F.group_norm(xr.permute(0, 2, 1), G, gr, br, 1e-5).permute(0, 2, 1)
    if silu:
        yr = F.silu(yr)
    dy, dk = rnd(B, HW, C, seed=4), rnd(B, HW, C, seed=5)
    (yr * dy.double() + xr * dk.double()).sum().backward()
    gm = torch.nn.Parameter(gam.to(dev)); gm.grad = torch.zeros_like(gm)
    bm = torch.nn.Parameter(bet.to(dev)); bm.grad = torch.zeros_like(bm)
    xd = x.to(dev).requires_grad_()
    y, xk = ops.group_norm(xd, gm, bm, G, 1e-5, silu, fork=True)
    assert y.dtype == F32
    close(y, yr, TOL, 'fwd')
    (y * dy.to(dev) + xk * dk.to(dev)).sum().backward()
    close(xd.grad, xr.grad, 5e-5, 'dx (+ fused residual gradient)')
    close(gm.grad, gr.grad, 5e-5, 'dgamma')
    close(bm.grad, br.grad, 5e-5, 'dbeta')


@pytest.mark.parametrize('rows,C', [(100, 320), (4096, 640), (257, 1280), (64, 32)])
def test_layernorm_f32(dev, rows, C):
    from sid_lsg_amd import ops
    x = rnd(rows, C, seed=1) * 2 - 0.5
    gam, bet = rnd(C, seed=2) * 0.5 + 1, rnd(C, seed=3) * 0.3
    xr, gr, br = (t.double().requires_grad_() for t in (x, gam, bet))
    yr = F.layer_norm(xr, (C,), gr, br, 1e-5)
    dy = rnd(rows, C, seed=4)
    yr.backward(dy.double())
    gm = torch.nn.Parameter(gam.to(dev)); gm.grad = torch.zeros_like(gm)
    bm = torch.nn.Parameter(bet.to(dev)); bm.grad = torch.zeros_like(bm)
    xd = x.to(dev).requires_grad_()
    y = ops.layer_norm(xd, gm, bm, 1e-5)
    close(y, yr, TOL, 'fwd')
    y.backward(dy.to(dev))
    close(xd.grad, xr.grad, 5e-5, 'dx')
    close(gm.grad, gr.grad, 5e-5, 'dgamma')
    close(bm.grad, br.grad, 5e-5, 'dbeta')


def _norm_f32_distinct(dev, run, c, rel, factor, what):
    """Distinct statistics per (sample, group) / per row (tests/norm_cases.py) in the fp32 mode: y and dx judged per block with `rel`,
    dgamma / dbeta globally, at `factor` times this file's operator tolerances.  Prints the figures (profiles/norm_offset_accuracy.txt)."""
    gm = torch.nn.Parameter(c['gam'].to(dev)); gm.grad = torch.zeros_like(gm)
    bm = torch.nn.Parameter(c['bet'].to(dev)); bm.grad = torch.zeros_like(bm)
    xd = c['x'].to(dev).requires_grad_()
    y = run(xd, gm, bm)
    assert y.dtype == F32
    y.backward(c['dy'].to(dev))
    ref = c['ref']
    errs = dict(y=rel(y, ref['y']), dx=rel(xd.grad, ref['dx']),
                dgamma=nc.global_rel_err(gm.grad, ref['dgamma']), dbeta=nc.global_rel_err(bm.grad, ref['dbeta']))
    print(f'NORM_ACCURACY hip_fp32 {what} ' + ' '.join(f'{k}={v:.3g}' for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= factor * nc.TOL_F32[k], f'{what}: {k} rel err {v:.3g} > {factor * nc.TOL_F32[k]:.3g}'


@pytest.mark.parametrize('name,offsets,factor', nc.OFFSET_SETS_F32, ids=[s[0] for s in nc.OFFSET_SETS_F32])
@pytest.mark.parametrize('case', nc.GN_CASES_F32, ids=nc.gn_id)
def test_groupnorm_f32_distinct_groups(dev, case, name, offsets, factor):
    """Per-group |mean| / std up to 30 at the operator tolerances (2e-5 forward, 5e-5 backward) and up to 100 at 4x (an error relative
    to |mean| grows linearly with the offset; torch's own fp32 result does, tests/test_norm_cases_host.py): the statistics must not be
    formed as sumsq / n - mean^2 from raw fp32 sums, which loses |mean / std|^2 * 2^-24 of the variance."""
    from sid_lsg_amd import ops
    B, HW, C, G, silu, eps, fork = case
    c = nc.gn_case(case, offsets, F32)
    assert TOL == nc.TOL_F32['y']
    _norm_f32_distinct(dev, lambda xd, gm, bm: ops.group_norm(xd, gm, bm, G, eps, silu), c, lambda got, ref: nc.group_rel_err(got, ref, G),
                       factor, f'gn {nc.gn_id(case)} {name}')


@pytest.mark.parametrize('name,offsets,factor', nc.OFFSET_SETS_F32, ids=[s[0] for s in nc.OFFSET_SETS_F32])
@pytest.mark.parametrize('rows,C', nc.LN_CASES_F32)
def test_layernorm_f32_distinct_rows(dev, rows, C, name, offsets, factor):
    from sid_lsg_amd import ops
    c = nc.ln_case((rows, C), offsets, F32)
    _norm_f32_distinct(dev, lambda xd, gm, bm: ops.layer_norm(xd, gm, bm, 1e-5), c, nc.row_rel_err, factor, f'ln {rows}-{C} {name}')


def attn_ref(q, k, v, heads):
    B, Nq, C = q.shape
    d = C // heads
    qh, kh, vh = (t.reshape(B, -1, heads, d).transpose(1, 2) for t in (q, k, v))
    p = torch.softmax(qh @ kh.transpose(-1, -2) * d ** -0.5, -1)
    return (p @ vh).transpose(1, 2).reshape(B, Nq, C)


@pytest.mark.parametrize('B,N,heads,D', [(2, 64, 2, 16), (1, 256, 4, 32), (2, 200, 2, 40), (1, 1000, 2, 64), (2, 256, 2, 80),
                                         (1, 320, 2, 160), (1, 2048, 1, 40)])
def test_self_attention_f32(dev, B, N, heads, D):
    from sid_lsg_amd import ops
    C = heads * D
    qkv = rnd(B, N, 3 * C, seed=1)
    qkv[0, 3, :C] *= 6.0           # one dominant query / key pair: exercises the running-max rescale
    qkv[0, 5, C:2 * C] *= 6.0
    r = qkv.double().requires_grad_()
    yr = attn_ref(r[..., :C], r[..., C:2 * C], r[..., 2 * C:], heads)
    do = rnd(B, N, C, seed=2)
    yr.backward(do.double())
    qd = qkv.to(dev).requires_grad_()
    y = ops.self_attention(qd, heads)
    assert y.dtype == F32
    close(y, yr, TOL, 'fwd')
    y.backward(do.to(dev))
    close(qd.grad[..., :C], r.grad[..., :C], 5e-5, 'dq')
    close(qd.grad[..., C:2 * C], r.grad[..., C:2 * C], 5e-5, 'dk')
    close(qd.grad[..., 2 * C:], r.grad[..., 2 * C:], 5e-5, 'dv')


@pytest.mark.parametrize('B,N,L,heads,D', [(2, 256, 77, 2, 40), (2, 64, 13, 4, 32), (2, 100, 77, 2, 160)])
def test_cross_attention_f32(dev, B, N, L, heads, D):
    from sid_lsg_amd import ops
    C = heads * D
    q, kv = rnd(B, N, C, seed=1), rnd(B, L, 2 * C, seed=3)
    qr, kr = q.double().requires_grad_(), kv.double().requires_grad_()
    yr = attn_ref(qr, kr[..., :C], kr[..., C:], heads)
    do = rnd(B, N, C, seed=2)
    yr.backward(do.double())
    qd, kd = q.to(dev).requires_grad_(), kv.to(dev).requires_grad_()
    y = ops.cross_attention(qd, kd, heads)
    close(y, yr, TOL, 'fwd')
    y.backward(do.to(dev))
    close(qd.grad, qr.grad, 5e-5, 'dq')
    close(kd.grad, kr.grad, 5e-5, 'dkv')


def test_small_ops_f32(dev):
    from sid_lsg_amd import ops
    h = rnd(300, 2 * 640, seed=1)
    hr = h.double().requires_grad_()
    a, g = hr.chunk(2, -1)
    yr = a * F.gelu(g)
    dy = rnd(300, 640, seed=2)
    yr.backward(dy.double())
    hd = h.to(dev).requires_grad_()
    y = ops.geglu(hd)
    y.backward(dy.to(dev))
    close(y, yr, TOL, 'geglu')
    close(hd.grad, hr.grad, TOL, 'geglu bwd')
    x = rnd(64, 1280, seed=3)
    xr = x.double().requires_grad_()
    F.silu(xr).backward(dy.double()[:64].repeat(1, 2))
    xd = x.to(dev).requires_grad_()
    ops.silu(xd).backward(dy.to(dev)[:64].repeat(1, 2))
    close(xd.grad, xr.grad, TOL, 'silu bwd')
    a2, b2 = rnd(2, 5, 7, 64, seed=4), rnd(2, 5, 7, 32, seed=5)
    ad, bd = a2.to(dev).requires_grad_(), b2.to(dev).requires_grad_()
    c = ops.concat_channels(ad, bd)
    assert torch.equal(c.cpu(), torch.cat([a2, b2], -1))
    c.backward(c)
    assert torch.equal(ad.grad.cpu(), a2) and torch.equal(bd.grad.cpu(), b2)
    assert torch.equal(ops.add(ad.detach(), ad.detach()).cpu(), a2 + a2)
    t = torch.tensor([0, 20, 625, 979], device=dev)
    e = ops.timestep_embed(t, 320, F32).double().cpu()
    i = torch.arange(160, dtype=F64)
    ang = t.cpu().double()[:, None] * torch.exp(-np.log(10000.0) * i / 160)[None]
    close(e, torch.cat([ang.cos(), ang.sin()], 1), 2e-4, 'timestep embedding')      # fp32 sin/cos of arguments up to ~1e3


# ---- composed path ---------------------------------------------------------------------------------------------------
def make_pair(cfg_name, dev, seed=1234):
    from oracle import fixtures
    from sid_lsg_amd.unet import CONFIGS, HipUNet2DCondition
    ref = fixtures.make_unet(cfg_name, seed=seed)
    hip = HipUNet2DCondition(CONFIGS[cfg_name], compute_dtype=F32).materialize(dev, source=ref.state_dict())
    return ref, hip


@pytest.mark.parametrize('cfg_name,lat', [('tiny', 16), ('tiny40', 8), ('tiny21', 16)])
def test_unet_forward_backward_f32(dev, cfg_name, lat):
    from oracle.unet_ref import CONFIGS as RC
    ref, hip = make_pair(cfg_name, dev)
    cfg = RC[cfg_name]
    g = torch.Generator().manual_seed(0)
    B = 2
    x = torch.randn(B, 4, lat, lat, generator=g)
    t = torch.tensor([625, 37])
    ctx = torch.randn(B, cfg.text_len, cfg.cross_attention_dim, generator=g)
    xr = x.clone().requires_grad_()
    ref.requires_grad_(True)
    yr = ref(xr, t, encoder_hidden_states=ctx).sample
    hip.requires_grad_(True)
    xd = x.to(dev).requires_grad_()
    y = hip(xd, t.to(dev), encoder_hidden_states=ctx.to(dev)).sample
    e = close(y, yr, 1e-4, 'UNet forward')
    dy = torch.randn(B, 4, lat, lat, generator=g)
    yr.backward(dy)
    y.backward(dy.to(dev))
    e2 = close(xd.grad, xr.grad, 2e-4, 'input gradient')
    ref_p = dict(ref.named_parameters())
    worst = 0.0
    for name, p in hip.named_parameters():
        gr = ref_p[name].grad
        # + 1e-3: gradients that are exactly zero in exact arithmetic (q / k projections of a 1-token attention at the 1x1
        # mid block of the lat=8 case) are ~1e-7 rounding noise on both sides
        err = ((p.grad.detach().float().cpu() - gr).norm() / (gr.norm() + 1e-3)).item()
        worst = max(worst, err)
        assert err < 1e-3, f'param grad {name}: rel l2 {err:.3g}'
    print(f'{cfg_name} fp32: fwd {e:.2e}  dx {e2:.2e}  worst param-grad rel l2 {worst:.2e}')


def _iteration_f32(dev, cfg_name, lat, b, rounds, lr, kappa, alpha, iters):
    from oracle import fixtures, sid_ref
    from oracle.scheduler_ref import DDPMSchedulerRef
    from oracle.unet_ref import CONFIGS as RC
    from sid_lsg_amd.optim import FusedAdamEMA
    from sid_lsg_amd.scheduler import DDPMScheduler
    from sid_lsg_amd.sid_step import SiDStep
    from sid_lsg_amd.unet import CONFIGS, HipUNet2DCondition
    cfg = RC[cfg_name]
    phi_r = fixtures.make_unet(cfg_name).eval().requires_grad_(False)
    psi_r = fixtures.make_unet(cfg_name, seed=77).requires_grad_(False)
    G_r = copy.deepcopy(phi_r)
    Gema_r = copy.deepcopy(G_r)
    nets_r = dict(true_score=phi_r, fake_score=psi_r, G=G_r, G_ema=Gema_r)
    mk = lambda r: HipUNet2DCondition(CONFIGS[cfg_name], compute_dtype=F32).materialize(dev, source=r.state_dict())   # noqa: E731
    phi, psi, G, G_ema = mk(phi_r), mk(psi_r), mk(G_r), mk(G_r)
    step = SiDStep(G, psi, phi, G_ema, DDPMScheduler().to(dev), FusedAdamEMA(psi.parameters(), lr=lr), FusedAdamEMA(G.parameters(), lr=lr),
                   alpha=alpha, cfg_train_fake=kappa, cfg_eval_fake=kappa, cfg_eval_real=kappa, batch_gpu_total=b * rounds, init_timestep=625)
    st = dict(fake_score=[{} for _ in psi_r.parameters()], G=[{} for _ in G_r.parameters()])
    hp = dict(alpha=alpha, kappa1=kappa, kappa2=kappa, kappa4=kappa, ls=1.0, lsg=1.0, batch_gpu_total=b * rounds, lr=lr, glr=lr,
              betas=(0.0, 0.999), eps=1e-8, init_t=625, batch_size=b * rounds, ema_halflife_kimg=50, ema_rampup_ratio=0.05)
    gen = torch.Generator().manual_seed(5)
    cur = 0
    for it in range(iters):
        inputs = dict(A=[], B=[])
        for ph in ('A', 'B'):
            for _ in range(rounds):
                inputs[ph].append(dict(z=torch.randn(b, 4, lat, lat, generator=gen), noise=torch.randn(b, 4, lat, lat, generator=gen),
                                       t=torch.randint(20, 980, (b,), generator=gen),
                                       cond=torch.randn(b, cfg.text_len, cfg.cross_attention_dim, generator=gen),
                                       uncond=torch.randn(1, cfg.text_len, cfg.cross_attention_dim, generator=gen).expand(b, -1, -1).contiguous()))
        hp['cur_nimg'] = cur
        out_r = sid_ref.sid_iteration_ref(nets_r, st, DDPMSchedulerRef(), inputs, hp)
        dinp = {ph: [{k: v.to(dev) for k, v in r.items()} for r in inputs[ph]] for ph in inputs}
        lf, lg = step.iteration(dinp, ema_beta=sid_ref.ema_beta_ref(b * rounds, cur, 50, 0.05))
        rf = abs(float(lf) - out_r['loss_fake']) / abs(out_r['loss_fake'])
        rg = abs(float(lg) - out_r['loss_G']) / abs(out_r['loss_G'])
        print(f'{cfg_name} kappa {kappa} iter {it} fp32: loss_fake {float(lf):.6f} vs {out_r["loss_fake"]:.6f} ({rf:.1e}); '
              f'loss_G {float(lg):.6f} vs {out_r["loss_G"]:.6f} ({rg:.1e})')
        assert rf < 1e-3 and rg < 1e-3, 'north_star: loss within 1e-3 of the reference fp32 path'
        cur += b * rounds
    # Adam(beta1 = 0) moves each weight by ~lr * sign(g): with fp32 gradients the signs agree except where g ~ 0
    for net, net_r, seed in ((psi, psi_r, 77), (G, G_r, 1234)):
        init = dict(fixtures.make_unet(cfg_name, seed=seed).named_parameters())
        ref_p = dict(net_r.named_parameters())
        agree = total = 0
        for n, p in net.named_parameters():
            du, dr = (p.detach().cpu() - init[n]).flatten(), (ref_p[n].detach() - init[n]).flatten()
            big = dr.abs() > 0.5 * lr
            agree += int((torch.sign(du[big]) == torch.sign(dr[big])).sum())
            total += int(big.sum())
        print(f'update-sign agreement {agree / max(total, 1):.5f} over {total} weights')
        assert agree / max(total, 1) > 0.999
    ema_r = dict(Gema_r.named_parameters())
    for n, p in G_ema.named_parameters():
        if n in ('conv_in.weight', 'conv_out.bias'):
            close(p, ema_r[n], 1e-4, f'EMA {n}')


@pytest.mark.parametrize('kappa,alpha', [(1.5, 1.0), (1.0, 1.2), (4.5, 1.0)])
def test_sid_iteration_f32_matches_oracle(dev, kappa, alpha):
    _iteration_f32(dev, 'tiny', lat=8, b=2, rounds=2, lr=2e-5, kappa=kappa, alpha=alpha, iters=2)


@pytest.mark.parametrize('name', ['k15_a1', 'k1_a12', 'k45_a1'])
def test_product_loop_f32_matches_reference_golden(dev, golden_dir, tmp_path, name):
    """`training_loop(**c)` in fp32 mode against the loss curves of the UNMODIFIED reference training_loop: 1e-3 on every
    recorded loss of every iteration (north_star), plus the weights the reference ended with."""
    from oracle import fixtures
    from sid_lsg_amd import training_loop as tl
    from sid_lsg_amd.scheduler import DDPMScheduler
    from sid_lsg_amd.unet import CONFIGS, HipUNet2DCondition
    from test_gpu_unet import _loop_kwargs_from_golden
    g = np.load(os.path.join(golden_dir, f'loop_{name}.npz'))
    cfg = str(g['cfg'])
    pdir = tmp_path / 'prompts'
    pdir.mkdir()
    (pdir / 'aesthetics_6_plus.txt').write_text('\n'.join(str(p) for p in g['prompts']) + '\n')
    run = tmp_path / 'run'
    run.mkdir()

    def factory(**kw):
        ref, vae, _, te, tok = fixtures.factory(cfg)
        unet = HipUNet2DCondition(CONFIGS[cfg], compute_dtype=kw['compute_dtype']).materialize(dev, source=ref.state_dict())
        return unet, vae, DDPMScheduler().to(dev), te.to(dev), tok
    losses = []
    kw = _loop_kwargs_from_golden(g, run, pdir, dev)
    kw['network_kwargs']['compute_dtype'] = 'fp32'
    saved = tl.load_sd15
    try:
        tl.load_sd15 = factory
        out = tl.training_loop(on_iteration=lambda it, lf, lg: losses.extend([lf, lg]), **kw)
    finally:
        tl.load_sd15 = saved
    got, ref = np.array(losses), g['loss_values']
    rel = np.abs(got - ref) / np.abs(ref)
    print(f'loop_{name} fp32: product {got} reference {ref} rel {rel}')
    assert got.shape == ref.shape and rel.max() < 1e-3
    # the weights the reference ended with: every Adam(beta1=0) step moves a weight by ~ +-lr, so a differing gradient
    # SIGN shows as an error of 2*lr; with fp32 gradients that only happens where the gradient is ~0
    lr = float(g['kw_lr'])
    for net, key, pname in ((out['G'], 'G_conv_in_w', 'conv_in.weight'), (out['fake_score'], 'fake_conv_in_w', 'conv_in.weight'),
                            (out['G'], 'G_last_b', 'conv_out.bias')):
        d = (dict(net.named_parameters())[pname].detach().cpu() - torch.from_numpy(g[key])).abs()
        frac = float((d < 0.05 * lr).float().mean())
        print(f'{key}: {frac:.4f} of the weights within 0.05 lr of the reference, max diff {float(d.max()) / lr:.2f} lr')
        assert frac > 0.98 and float(d.max()) <= 2.1 * lr * int(g['kw_iterations'])
