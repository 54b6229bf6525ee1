"""Grouped launches for e4m3 networks (include/sidlsg_hip.h "Grouped forms of the e4m3 entry points"): the fake-score network and the
teacher of `--teacher-weights fp8-frozen` as ONE pass over the stacked batch, on the MX-fp8 / fp8-weight kernels.

What is pinned, level by level:
  * kernels: sidlsg_{gemm,conv3x3}_{mx8,fp8w}_g2 and the two e4m3 norms against two ordinary launches on the halves.  Where the
    grouped launch and the single launches take the same split-K decision (the host rule of launch_gemm_mx8, restated in
    mx8_splits below; the fp8w kernels never split) the bits must be EQUAL; where the decisions differ only the fp32 summation
    order does: 1e-4 of the maximum with fp32 output, the 1e-2 of tests/test_gpu_grouped.py::same_or_close with bf16 output;
  * nodes: ops.norm_linear_mx8 / ops.norm_conv_mx8 inside dual_networks against the two single-network calls, outputs and input
    gradients, with and without fork;
  * network: HipUNet2DCondition.forward_pair of two e4m3 networks against the two single e4m3 forwards, bounded by a fifth of
    the e4m3 quantisation deviation measured in the same test;
  * step: one SiDStep iteration in the fp8-frozen arrangement, grouped against two-stream, bounded by the distance of the
    e4m3 step from the bf16 step."""
import contextlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from sid_lsg_amd._lib import lib
    lib.load()
    return torch.device('cuda:0')


def rnd(*shape, seed=0, scale=1.0, dev=None):
    g = torch.Generator().manual_seed(seed)
    t = (torch.randn(*shape, generator=g) * scale).to(BF16)
    return t.to(dev) if dev is not None else t


def P(t):
    return torch.nn.Parameter(t, requires_grad=False)


def mx8_splits(m_tiles, n, nk, m_total, ws_bytes=512 << 20):
    """K-tiles per split that launch_gemm_mx8 picks (0: no split-K) for m_tiles x n/160 output tiles and nk K-tiles of 128."""
    tiles = m_tiles * (n // 160)
    if not (tiles < 384 and nk >= 16 and m_total * n * 8 <= ws_bytes):
        return 0
    splits = min((512 + tiles - 1) // tiles, ws_bytes // (m_total * n * 4), nk // 4, 16)
    return (nk + splits - 1) // splits if splits >= 2 else 0


def check_contraction(got, ref, same_decision, what):
    """The agreement rule of the module docstring; returns how the shape fared (printed by the caller)."""
    if same_decision:
        assert torch.equal(got, ref), f'{what}: same split-K decision, so the grouped launch must reproduce the bits of the two ordinary launches'
        return 'same split-K decision: bit-equal'
    err = float((got.float() - ref.float()).abs().max() / (ref.float().abs().max() + 1e-12))
    tol = 1e-4 if got.dtype == F32 else 1e-2
    assert err < tol, f'{what}: grouped launch differs from the two ordinary launches by {err:.3g} of max (bound {tol:g})'
    return f'different split-K decisions: within {err:.1e} of max'


# ---------------------------------------------------------------------------------------------------------------- kernels
# (M_half, N, K): one tile per set; halves that are no multiple of the 128-row tile (the second set starts mid-tile in row terms);
# 2 x 77 text rows; K below one K-tile; split-K (fewer than 384 tiles, 45 K-tiles: both grids get 5 K-tiles per split); split-K where the
# grouped grid of 80 tiles gets 10 K-tiles per split and each half's 40 tiles get 5 (the tolerance branch of the agreement rule)
@pytest.mark.parametrize('Mh,N,K', [(128, 160, 128), (300, 160, 128), (154, 640, 768), (130, 480, 48), (64, 640, 5760), (1280, 640, 8192)])
@pytest.mark.parametrize('epi', ['none', 'bias', 'bias+res', 'f32'])
def test_gemm_mx8_g2_equals_two_launches(dev, Mh, N, K, epi):
    from sid_lsg_amd import ops
    a8 = ops.cast_fp8(rnd(2 * Mh, K, seed=1, dev=dev))
    w = [ops.Fp8Weight(rnd(N, K, seed=s, scale=K ** -0.5, dev=dev)) for s in (2, 3)]
    b = [rnd(N, seed=s, dev=dev).float() for s in (4, 5)] if epi != 'none' else None
    res = rnd(2 * Mh, N, seed=6, dev=dev) if epi == 'bias+res' else None
    f32 = epi == 'f32'
    got = ops.gemm_mx8(a8, ops.Pair(*w), bias=ops.Pair(*b) if b else None, res=res, out_f32=f32)
    half = lambda h, ws: ops.gemm_mx8(a8[h * Mh:(h + 1) * Mh], w[ws], bias=b[ws] if b else None,      # noqa: E731
                                      res=res[h * Mh:(h + 1) * Mh] if res is not None else None, out_f32=f32)
    ref = torch.cat([half(0, 0), half(1, 1)])
    mt, nk = (Mh + 127) // 128, (K + 127) // 128
    same = mx8_splits(2 * mt, N, nk, 2 * Mh) == mx8_splits(mt, N, nk, Mh)
    how = check_contraction(got, ref, same, f'gemm_mx8 {Mh}x{N}x{K} {epi}')
    assert got.dtype == (F32 if f32 else BF16)
    assert not torch.equal(got[Mh:], half(1, 0)), 'the second half must have used the second weight set'
    print(f'gemm_mx8_g2 2x{Mh} x {N} x {K} [{epi}] split-K kt/split {mx8_splits(2 * mt, N, nk, 2 * Mh)}: {how}')


# (B_half, H, W, Cin, Cout, full epilogue): halves of 96 / 63 pixels (set boundaries inside a tile; 48 channels: a partial chunk); Cin = 320
# (128 + 128 + 64 channel chunks) with split-K, bias + rowvec + res
@pytest.mark.parametrize('Bh,H,W,Cin,Cout,full', [(1, 8, 12, 128, 160, False), (1, 9, 7, 48, 160, False), (2, 16, 16, 320, 320, True)])
def test_conv3x3_mx8_g2_equals_two_launches(dev, Bh, H, W, Cin, Cout, full):
    from sid_lsg_amd import ops
    x8 = ops.cast_fp8(rnd(2 * Bh, H, W, Cin, seed=1, dev=dev))
    w = [ops.Fp8Weight(rnd(Cout, 9 * Cin, seed=s, scale=(9 * Cin) ** -0.5, dev=dev)) for s in (2, 3)]
    b = [rnd(Cout, seed=s, dev=dev).float() for s in (4, 5)]
    rv = rnd(2 * Bh, Cout, seed=6, dev=dev).float() if full else None
    res = rnd(2 * Bh, H, W, Cout, seed=7, dev=dev) if full else None
    got = ops.conv3x3_mx8(x8, ops.Pair(*w), bias=ops.Pair(*b), res=res, rowvec=rv)
    half = lambda h, ws: ops.conv3x3_mx8(x8[h * Bh:(h + 1) * Bh], w[ws], bias=b[ws], res=res[h * Bh:(h + 1) * Bh] if full else None,      # noqa: E731
                                         rowvec=rv[h * Bh:(h + 1) * Bh] if full else None)
    ref = torch.cat([half(0, 0), half(1, 1)])
    Mh = Bh * H * W
    mt, nk = (Mh + 127) // 128, 9 * ((Cin + 127) // 128)
    same = mx8_splits(2 * mt, Cout, nk, 2 * Mh) == mx8_splits(mt, Cout, nk, Mh)
    how = check_contraction(got, ref, same, f'conv3x3_mx8 {Bh}x{H}x{W} {Cin}->{Cout}')
    assert not torch.equal(got[Bh:], half(1, 0)), 'the second half must have used the second weight set'
    print(f'conv3x3_mx8_g2 B=2x{Bh} {H}x{W} {Cin}->{Cout} full={full} split-K kt/split {mx8_splits(2 * mt, Cout, nk, 2 * Mh)}: {how}')


# the shapes the tiny networks (80-channel stages, ragged N) and SIDLSG_MX8=0 send to the fp8-weight kernels.  K = 72 is no multiple of 16: the
# format does not take it (ops.Fp8Weight, sidlsg_gemm_fp8w) -- the grouped entry point must refuse it like the ordinary one; K = 80 is the
# nearest contraction length with the same ragged N that it does take
@pytest.mark.parametrize('Mh,N,K', [(300, 136, 72), (300, 136, 80), (154, 240, 80)])
@pytest.mark.parametrize('epi', ['none', 'bias+res', 'bias+rowvec'])
def test_gemm_fp8w_g2_equals_two_launches(dev, Mh, N, K, epi):
    from sid_lsg_amd import ops
    from sid_lsg_amd._lib import lib
    a = rnd(2 * Mh, K, seed=1, dev=dev)
    if K % 16:
        with pytest.raises(RuntimeError):
            ops.Fp8Weight(rnd(N, K, seed=2, dev=dev))
        q, sc, out = torch.zeros(N, K, dtype=torch.uint8, device=dev), torch.ones(N, device=dev), torch.empty(2 * Mh, N, dtype=BF16, device=dev)
        tail = (None, 0, None, 0, 1, 2 * Mh, N, K, 1.0, 0, None)      # res, ldres, rowvec, ld_rowvec, rows_per_batch, M, N, K, alpha, flags, stream
        assert lib.sidlsg_gemm_fp8w.raw(a.data_ptr(), K, q.data_ptr(), sc.data_ptr(), out.data_ptr(), N, None, *tail) != 0
        assert lib.sidlsg_gemm_fp8w_g2.raw(a.data_ptr(), K, q.data_ptr(), sc.data_ptr(), q.data_ptr(), sc.data_ptr(), out.data_ptr(), N, None, None, *tail) != 0
        return
    w = [ops.Fp8Weight(rnd(N, K, seed=s, scale=K ** -0.5, dev=dev)) for s in (2, 3)]
    b = [rnd(N, seed=s, dev=dev).float() for s in (4, 5)] if epi != 'none' else None
    res = rnd(2 * Mh, N, seed=6, dev=dev) if epi == 'bias+res' else None
    rpb = 77 if Mh % 77 == 0 else 1
    rv = rnd(2 * Mh // rpb, N, seed=7, dev=dev).float() if epi == 'bias+rowvec' else None
    got = ops.gemm(a, ops.Pair(*w), bias=ops.Pair(*b) if b else None, res=res, rowvec=rv, rows_per_batch=rpb)
    half = lambda h, ws: ops.gemm(a[h * Mh:(h + 1) * Mh], w[ws], bias=b[ws] if b else None, res=res[h * Mh:(h + 1) * Mh] if res is not None else None,      # noqa: E731
                                  rowvec=rv[h * Mh // rpb:(h + 1) * Mh // rpb] if rv is not None else None, rows_per_batch=rpb)
    how = check_contraction(got, torch.cat([half(0, 0), half(1, 1)]), True, f'gemm_fp8w {Mh}x{N}x{K} {epi}')      # (the fp8w kernels never split K)
    assert not torch.equal(got[Mh:], half(1, 0)), 'the second half must have used the second weight set'
    print(f'gemm_fp8w_g2 2x{Mh} x {N} x {K} [{epi}]: {how}')


@pytest.mark.parametrize('Bh,H,W,Cin,Cout,stride,ups', [(1, 10, 6, 80, 136, 2, 0), (1, 8, 12, 80, 80, 1, 1), (2, 5, 7, 80, 240, 1, 0)])
def test_conv3x3_fp8w_g2_equals_two_launches(dev, Bh, H, W, Cin, Cout, stride, ups):
    from sid_lsg_amd import ops
    Hs, Ws = (H // 2, W // 2) if ups else (H, W)
    x = rnd(2 * Bh, Hs, Ws, Cin, seed=1, dev=dev)
    w = [ops.Fp8Weight(rnd(Cout, 9 * Cin, seed=s, scale=(9 * Cin) ** -0.5, dev=dev)) for s in (2, 3)]
    b = [rnd(Cout, seed=s, dev=dev).float() for s in (4, 5)]
    rv = rnd(2 * Bh, Cout, seed=6, dev=dev).float()
    got = ops.conv3x3(x, ops.Pair(*w), bias=ops.Pair(*b), rowvec=rv, stride=stride, ups=ups)
    half = lambda h, ws: ops.conv3x3(x[h * Bh:(h + 1) * Bh], w[ws], bias=b[ws], rowvec=rv[h * Bh:(h + 1) * Bh], stride=stride, ups=ups)      # noqa: E731
    how = check_contraction(got, torch.cat([half(0, 0), half(1, 1)]), True, f'conv3x3_fp8w {Bh}x{H}x{W} {Cin}->{Cout} s{stride} u{ups}')
    assert not torch.equal(got[Bh:], half(1, 0)), 'the second half must have used the second weight set'
    print(f'conv3x3_fp8w_g2 B=2x{Bh} {H}x{W} {Cin}->{Cout} s{stride} u{ups}: {how}')


def test_mixed_weight_pairs_are_refused(dev):
    from sid_lsg_amd import ops
    a = rnd(32, 80, seed=1, dev=dev)
    w = rnd(136, 80, seed=2, dev=dev)
    with pytest.raises(RuntimeError, match='both'):
        ops.gemm(a, ops.Pair(ops.Fp8Weight(w), w))


@pytest.mark.parametrize('Bh,HW,C,G', [(1, 64, 160, 8), (2, 256, 320, 32)])
@pytest.mark.parametrize('silu', [True, False])
def test_groupnorm_fp8_g2_equals_two_launches(dev, Bh, HW, C, G, silu):
    from sid_lsg_amd import ops
    from sid_lsg_amd._lib import lib
    x = rnd(2 * Bh, HW, C, seed=1, dev=dev) * 2 + 0.5
    g0, g1, be0, be1 = [rnd(C, seed=s, dev=dev).float() + (1.0 if s < 4 else 0.0) for s in (2, 3, 4, 5)]
    y8, stats, n = ops.groupnorm_fp8_g2(x, (g0, g1), (be0, be1), G, 1e-5, silu)

    def single(xh, g, be):
        ws = torch.empty(lib.sidlsg_groupnorm_ws_floats.raw(Bh, HW, C, G), device=dev, dtype=F32)
        y, st = torch.empty(xh.shape, device=dev, dtype=torch.uint8), torch.empty(Bh, G, 2, device=dev, dtype=F32)
        lib.sidlsg_groupnorm_fwd_fp8(xh.data_ptr(), g.data_ptr(), be.data_ptr(), y.data_ptr(), st.data_ptr(), ws.data_ptr(), Bh, HW, C, G, 1e-5,
                                     int(silu), torch.cuda.current_stream().cuda_stream)
        return y, st
    (ya, sa), (yb, sb) = single(x[:Bh].contiguous(), g0, be0), single(x[Bh:].contiguous(), g1, be1)
    assert torch.equal(y8, torch.cat([ya, yb])) and torch.equal(stats, torch.cat([sa, sb])), 'per-sample op: e4m3 bytes and statistics must be equal'
    assert not torch.equal(y8[Bh:], single(x[Bh:].contiguous(), g0, be0)[0]), 'the second half must have used the second parameter set'


# 77 rows per half: no multiple of the kernel's rows per wave -- ops runs the halves as two ordinary launches (ops._layernorm_fwd, as for ops.layer_norm);
# 256: the grouped launch
@pytest.mark.parametrize('rows_h,C', [(77, 160), (256, 320)])
def test_layernorm_fp8_g2_equals_two_launches(dev, rows_h, C):
    from sid_lsg_amd import ops
    from sid_lsg_amd._lib import lib
    x = rnd(2 * rows_h, C, seed=1, dev=dev) * 2 + 0.5
    g0, g1, be0, be1 = [rnd(C, seed=s, dev=dev).float() + (1.0 if s < 4 else 0.0) for s in (2, 3, 4, 5)]
    y8, stats, grouped = ops.layernorm_fp8_g2(x, (g0, g1), (be0, be1), 1e-5)
    assert grouped == (rows_h % 16 == 0)

    def single(xh, g, be):
        y, st = torch.empty(xh.shape, device=dev, dtype=torch.uint8), torch.empty(rows_h, 2, device=dev, dtype=F32)
        lib.sidlsg_layernorm_fwd_fp8(xh.data_ptr(), g.data_ptr(), be.data_ptr(), y.data_ptr(), st.data_ptr(), rows_h, C, 1e-5,
                                     torch.cuda.current_stream().cuda_stream)
        return y, st
    (ya, sa), (yb, sb) = single(x[:rows_h], g0, be0), single(x[rows_h:], g1, be1)
    assert torch.equal(y8, torch.cat([ya, yb])) and torch.equal(stats, torch.cat([sa, sb])), 'row-wise op: e4m3 bytes and statistics must be equal'
    assert not torch.equal(y8[rows_h:], single(x[rows_h:], g0, be0)[0]), 'the second half must have used the second parameter set'


# ------------------------------------------------------------------------------------------------------------------ nodes
def same_or_close(got, ref, what):      # the rule of tests/test_gpu_grouped.py for bf16 results
    if torch.equal(got, ref):
        return 'bit-equal'
    err = float((got.float() - ref.float()).abs().max() / (ref.float().abs().max() + 1e-12))
    assert err < 1e-2, f'{what}: grouped node differs from the two single-network calls by {err:.3g} of max'
    return f'within {err:.1e}'


def _node_sets(dev, C, N, conv, temb=False):
    from sid_lsg_amd import ops
    sets = []
    for s0 in (10, 20):
        K = 9 * C if conv else C
        w = rnd(N, K, seed=s0, scale=K ** -0.5, dev=dev)
        wt = ops.transpose_w(w.float().view(N, 9, C), N, C, 9) if conv else w.t().contiguous()
        sets.append(dict(gamma=P(rnd(C, seed=s0 + 1, dev=dev).float() + 1.0), beta=P(rnd(C, seed=s0 + 2, dev=dev).float()), w8=ops.Fp8Weight(w),
                         bias=P(rnd(N, seed=s0 + 3, dev=dev).float()), w16t=wt, weight=P(w.float())))
    a, b = sets
    return a, b, {id(a[k]): b[k] for k in a}


@pytest.mark.parametrize('form,Bh,HW,C,N', [('ln', 1, 256, 160, 480), ('ln', 2, 77, 320, 320), ('gn', 1, 64, 160, 160), ('gn', 2, 256, 320, 320)])
@pytest.mark.parametrize('fork', [True, False])
def test_norm_linear_mx8_under_dual_networks(dev, form, Bh, HW, C, N, fork):
    from sid_lsg_amd import ops
    a, b, pmap = _node_sets(dev, C, N, conv=False)
    groups = 0 if form == 'ln' else 32 if C == 320 else 8
    x = rnd(2 * Bh, HW, C, seed=1, dev=dev) * 2 + 0.5
    dy, dk = rnd(2 * Bh * HW, N, seed=2, dev=dev), rnd(2 * Bh, HW, C, seed=3, dev=dev)

    def run(sl, st, dual):
        xg = x[sl].clone().requires_grad_()
        with ops.dual_networks(pmap) if dual else contextlib.nullcontext():
            out = ops.norm_linear_mx8(xg, st['gamma'], st['beta'], 1e-5, st['w8'], st['bias'], st['w16t'], st['weight'], groups=groups, fork=fork)
        y, xk = out if fork else (out, None)
        rows = slice(sl.start * HW, sl.stop * HW)
        loss = (y.float() * dy[rows].float()).sum()
        if fork:
            loss = loss + (xk.float() * dk[sl].float()).sum()
        loss.backward()
        return y.detach(), xg.grad
    y, gx = run(slice(0, 2 * Bh), a, True)
    parts = [run(slice(0, Bh), a, False), run(slice(Bh, 2 * Bh), b, False)]
    print(f'norm_linear_mx8 {form} 2x{Bh}x{HW}x{C}->{N} fork={fork}: out {same_or_close(y, torch.cat([p[0] for p in parts]), "output")}, '
          f'dx {same_or_close(gx, torch.cat([p[1] for p in parts]), "input gradient")}')
    assert not torch.equal(y[Bh * HW:], run(slice(Bh, 2 * Bh), a, False)[0]), 'the second half must have used the second network'


@pytest.mark.parametrize('Bh,H,W,C,N,full', [(1, 8, 12, 160, 160, False), (2, 16, 16, 320, 320, True)])
@pytest.mark.parametrize('fork', [True, False])
def test_norm_conv_mx8_under_dual_networks(dev, Bh, H, W, C, N, full, fork):
    from sid_lsg_amd import ops
    a, b, pmap = _node_sets(dev, C, N, conv=True)
    groups = 32 if C == 320 else 8
    x = rnd(2 * Bh, H, W, C, seed=1, dev=dev) * 2 + 0.5
    dy, dk = rnd(2 * Bh, H, W, N, seed=2, dev=dev), rnd(2 * Bh, H, W, C, seed=3, dev=dev)
    rv = rnd(2 * Bh, N, seed=4, dev=dev).float() if full else None
    res = rnd(2 * Bh, H, W, N, seed=5, dev=dev) if full else None

    def run(sl, st, dual):
        xg = x[sl].clone().requires_grad_()
        rg = res[sl].clone().requires_grad_() if full else None
        with ops.dual_networks(pmap) if dual else contextlib.nullcontext():
            out = ops.norm_conv_mx8(xg, st['gamma'], st['beta'], 1e-5, groups, st['w8'], st['bias'], st['w16t'], st['weight'], res=rg,
                                    rowvec=rv[sl] if full else None, fork=fork)
        y, xk = out if fork else (out, None)
        loss = (y.float() * dy[sl].float()).sum()
        if fork:
            loss = loss + (xk.float() * dk[sl].float()).sum()
        loss.backward()
        return y.detach(), xg.grad, rg.grad if full else None
    y, gx, gr = run(slice(0, 2 * Bh), a, True)
    parts = [run(slice(0, Bh), a, False), run(slice(Bh, 2 * Bh), b, False)]
    print(f'norm_conv_mx8 2x{Bh}x{H}x{W} {C}->{N} full={full} fork={fork}: out {same_or_close(y, torch.cat([p[0] for p in parts]), "output")}, '
          f'dx {same_or_close(gx, torch.cat([p[1] for p in parts]), "input gradient")}')
    if full:
        assert torch.equal(gr, dy), 'the residual gradient is the output gradient'
    assert not torch.equal(y[Bh:], run(slice(Bh, 2 * Bh), a, False)[0]), 'the second half must have used the second network'


# ---------------------------------------------------------------------------------------------------------------- network
def test_forward_pair_of_e4m3_networks(dev):
    """tiny40 at latent 16 (MX stages of 160 / 320 channels, fp8-weight stages of 80): forward_pair(psi, phi) with phi on always-active e4m3 copies
    and psi on frozen_passes_only ones == the two single e4m3 forwards, to a fifth of the e4m3-vs-bf16 deviation d_q measured here."""
    from sid_lsg_amd import ops
    from sid_lsg_amd.unet import CONFIGS, HipUNet2DCondition
    cfg, lat, B = CONFIGS['tiny40'], 16, 2
    psi = HipUNet2DCondition(cfg).materialize(dev, seed=11).requires_grad_(False)
    phi = HipUNet2DCondition(cfg).materialize(dev, seed=12).requires_grad_(False)
    plain = HipUNet2DCondition(cfg).materialize(dev, seed=11).requires_grad_(False)      # a bf16 network for the mixed pair
    g = torch.Generator().manual_seed(0)
    x = torch.zeros(B, lat, lat, 8)
    x[..., :4] = torch.randn(B, lat, lat, 4, generator=g)
    x = x.to(dev).to(BF16)
    t = torch.randint(20, 980, (B,), generator=g).to(dev)
    ctx = torch.randn(B, cfg.text_len, cfg.cross_attention_dim, generator=g).to(dev).to(BF16)
    dy = torch.randn(2, B, lat * lat, 8, generator=g).to(dev)

    def rel(a, b):
        return float((a.float() - b.float()).norm() / (b.float().norm() + 1e-12))

    def singles():
        xb = x.clone().requires_grad_()
        with psi.fp8_forward():
            ra = psi.forward_nhwc(xb, t, ctx)
        rb = phi.forward_nhwc(xb, t, ctx)
        (ra * dy[0] + rb * dy[1]).sum().backward()
        return ra.detach(), rb.detach(), xb.grad

    def pair():
        xa = x.clone().requires_grad_()
        ea, eb = psi.forward_pair(phi, xa, t, ctx)
        (ea * dy[0] + eb * dy[1]).sum().backward()
        return ea.detach(), eb.detach(), xa.grad
    b16 = singles()                                        # both networks still bf16
    assert phi.enable_fp8_weights() > 0 and psi.enable_fp8_weights(frozen_passes_only=True) > 0
    mx = psi._flat['fp8_mx8']
    assert psi._flat['fp8_mx8'] and any(not ops.mx8_ok(q) for q, _ in psi._flat['fp8']), 'the configuration must exercise the MX and the fp8-weight kernels'
    slots_bf16 = lambda net: all(not isinstance(w, ops.Fp8Weight) for w in _forward_weights(net))      # noqa: E731
    assert slots_bf16(psi) and not slots_bf16(phi)
    f8 = singles()
    d_q = max(rel(f8[0], b16[0]), rel(f8[1], b16[1]))
    d_q_grad = rel(f8[2], b16[2])
    for round_ in ('first pass', 'after refresh_compute_weights'):
        got = pair()
        e = (rel(got[0], f8[0]), rel(got[1], f8[1]), rel(got[2], f8[2]))
        print(f'{round_}: d_q {d_q:.3e}  d_q_grad {d_q_grad:.3e}  grouped vs single e4m3: eps psi {e[0]:.3e}  eps phi {e[1]:.3e}  input gradient {e[2]:.3e}'
              f'  (bounds {max(2e-3, 0.2 * d_q):.3e} / {max(5e-3, 0.2 * d_q_grad):.3e})')
        assert max(e[0], e[1]) < max(2e-3, 0.2 * d_q)
        assert e[2] < max(5e-3, 0.2 * d_q_grad)
        assert rel(got[1], f8[0]) > 0.1, 'the second half must have been evaluated with the second network'
        assert slots_bf16(psi) and not any(m.mx8 for m in mx), "after the pass psi's modules point at their bf16 copies again"
        assert not slots_bf16(phi)
        psi.refresh_compute_weights()                      # re-quantises the e4m3 copies in place: the cached map stays valid
        phi.refresh_compute_weights()
    with pytest.raises(RuntimeError, match='e4m3'):
        plain.partner_map(phi)
    with pytest.raises(RuntimeError, match='e4m3'):
        phi.forward_pair(plain, x, t, ctx)


def _forward_weights(net):
    """What the converted layers' forward-weight attributes point at right now."""
    from sid_lsg_amd.unet import HConv3x3, HLinear
    out = []
    for mod in net.modules():
        if isinstance(mod, (HConv3x3, HLinear)) and not getattr(mod, '_fused_member', False):
            out.append(mod.w16)
        f = mod.__dict__.get('fused')
        if isinstance(f, dict):
            out.append(f['w16'])
    return out


# ------------------------------------------------------------------------------------------------------------------- step
def test_grouped_e4m3_pass_in_the_step(dev, monkeypatch):
    """One SiDStep iteration (tiny40, latent 16, b = 2, two accumulation rounds) from the same seeds: bf16 two-stream, fp8-frozen two-stream,
    fp8-frozen grouped.  The grouped e4m3 step must sit much closer to the two-stream e4m3 step than that sits to the bf16 step."""
    from sid_lsg_amd.optim import FusedAdamEMA
    from sid_lsg_amd.scheduler import DDPMScheduler
    from sid_lsg_amd.sid_step import SiDStep
    from sid_lsg_amd.unet import CONFIGS, HipUNet2DCondition
    cfg_name, lat, b, lr = 'tiny40', 16, 2, 2e-5
    cfg = CONFIGS[cfg_name]
    out = {}
    for run, (fp8, mode) in enumerate(((False, '0'), (True, '0'), (True, '1')), 1):
        monkeypatch.setenv('SIDLSG_GROUPED_FROZEN', mode)
        phi = HipUNet2DCondition(cfg).materialize(dev, seed=1).requires_grad_(False)
        psi = HipUNet2DCondition(cfg).materialize(dev, seed=2)
        G = phi.clone_network()
        G_ema = phi.clone_network(with_grad_buffers=False)
        if fp8:                                            # the arrangement of training_loop.py for teacher_weights = 'fp8-frozen'
            phi.enable_fp8_weights()
            for net in (psi, G):
                net.enable_fp8_weights(frozen_passes_only=True)
        step = SiDStep(G, psi, phi, G_ema, DDPMScheduler().to(dev), FusedAdamEMA(psi.parameters(), lr=lr), FusedAdamEMA(G.parameters(), lr=lr),
                       alpha=1.0, cfg_train_fake=1.5, cfg_eval_fake=1.5, cfg_eval_real=4.5, batch_gpu_total=2 * b, init_timestep=625)
        assert step._use_grouped(b) == (run == 3), f'run {run}: _use_grouped'
        gen = torch.Generator().manual_seed(3)
        inputs = {ph: [dict(z=torch.randn(b, 4, lat, lat, generator=gen).to(dev), noise=torch.randn(b, 4, lat, lat, generator=gen).to(dev),
                            t=torch.randint(20, 980, (b,), generator=gen).to(dev),
                            cond=torch.randn(b, cfg.text_len, cfg.cross_attention_dim, generator=gen).to(dev).to(BF16),
                            uncond=torch.randn(b, cfg.text_len, cfg.cross_attention_dim, generator=gen).to(dev).to(BF16)) for _ in range(2)]
                  for ph in ('A', 'B')}
        lf, lg = step.iteration(inputs, ema_beta=0.5)
        torch.cuda.synchronize()
        out[run] = dict(losses=np.array([float(lf), float(lg)]), G=G.flat_params.clone(), psi=psi.flat_params.clone(), ema=G_ema.flat_params.clone())
    r1, r2, r3 = out[1], out[2], out[3]
    d = np.abs(r2['losses'] - r1['losses']) / np.abs(r1['losses'])
    e = np.abs(r3['losses'] - r2['losses']) / np.abs(r2['losses'])
    print(f'losses bf16 {r1["losses"]}  e4m3 two-stream {r2["losses"]}  e4m3 grouped {r3["losses"]}  d {d}  grouped vs two-stream {e}')
    assert (e <= np.maximum(2e-3, 0.25 * d)).all()
    for k in ('G', 'psi', 'ema'):
        share = lambda x, y: float(((x[k] - y[k]).abs() > 0.5 * lr).float().mean())      # noqa: E731
        s32, s21 = share(r3, r2), share(r2, r1)
        dmax = float((r3[k] - r2[k]).abs().max())
        print(f'{k}: grouped vs two-stream: max weight difference {dmax / lr:.2f} lr, {s32:.4%} of the weights moved by more than lr / 2 '
              f'(e4m3 vs bf16: {s21:.4%})')
        assert s32 <= max(0.02, 0.5 * s21)
        assert dmax <= 4.02 * lr
