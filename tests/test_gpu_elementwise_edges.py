"""Edge tests of the kernels of sid_lsg_amd/csrc/elementwise.hip and optim.hip: the activations, GEGLU, the layout ops, colsum, the SiD
losses, the fused Adam / EMA step, the weight-preparation casts and transposes and the timestep embedding, at the shapes, values and
argument combinations where such kernels go wrong -- ragged last blocks, every bf16 bit pattern, the left tail of GELU, rows that
do not divide the block, empty chunks, NaNs in every input and wave, the grid-stride pass of the production sizes.

Cases, references, bounds and their derivation: tests/elementwise_cases.py; tests/test_elementwise_cases_host.py proves on the CPU
that references made wrong on purpose miss these bounds.  Every output is a view into a sentinel-filled buffer (Guarded): a write
outside the extent or an element never written fails the test.  `pytest -s` prints the largest error / bound of every kernel.

Where each gap of the older tests is closed:
  tail guard i >= n8, full blocks only        test_silu_and_add_shapes[2040 | 2056], test_geglu_shapes[7-24 | 257-8]
  randn only, error against the tensor max    test_activation_sweep (every bf16 pattern, per-element bound)
  gelu_fast's left tail, SiLU' zero, large x  test_activation_sweep[geglu_* | silu_bwd-*]
  colsum N < 2048 / lanes idle                test_colsum_exact[*-3-63-24 | 1-1-8 | 5-700-40]
  colsum second column pass, cc >= N8         test_colsum_exact[*-2-257-2056]
  colsum ldg > N                              every colsum case (ldg = N + 16, NaN in the pad)
  colsum chunk past the last row              test_colsum_exact[*-1-8193-8] (det: NaN-filled slab)
  sumpool2x2 / zero_insert2 on their own      test_sumpool2x2_exact, test_zero_insert2_exact (both parities of H, W, Ho, Wo)
  writes outside an extent                    Guarded.check in every test
  losses beyond block 0, 8 partials, S >= 9   test_generator_loss_cases / test_fake_score_loss_cases[S9-* | *-n2049-* | *-n4356-*]
  NaN in y_real / y_fake / later waves        the `nans` of elementwise_cases.LOSS_CASES (index 64, 255, last)
  w clip                                      the cases with -clip
  dropped sample's fake-loss gradient         loss_ratio: exactly 0
  optimizer grid-stride pass                  test_adam_ema_cases[*-4195507]
  exp_avg_sq / exp_avg never compared         test_adam_ema_cases: p, ema, v, m
  NaN / inf in the scalar tail                elementwise_cases.adam_special
  ema_beta < 0.5, zero_grad=False, beta1 != 0 with EMA and w16     ADAM_BETAS, ADAM_KEEP_GRAD_STEP, the 'everything' configuration
  scale_cast_ranges, cast tails, transpose_w16 off 64              test_scale_cast_ranges, test_cast_f32_bf16_*, test_transpose_w_*
"""
import pytest
import torch

import elementwise_cases as ec

pytestmark = pytest.mark.gpu

BF16, F32, F64 = ec.BF16, ec.F32, ec.F64
DTYPES = pytest.mark.parametrize('dtype', [BF16, F32], ids=['bf16', 'f32'])
NAN = float('nan')
_worst = {}


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs an MI355X')
    from sid_lsg_amd import ops
    ops.ensure_workspace('cuda')
    yield torch.device('cuda')
    for k in sorted(_worst):
        print(f'\nMEASURED {k}: {_worst[k]:.3f} of the bound', end='')


@pytest.fixture(params=['atomic', 'det'])
def mode(request, dev):
    from sid_lsg_amd import ops
    old = ops._det_explicit
    ops.set_deterministic(request.param == 'det')
    yield request.param
    ops.set_deterministic(old)


def _p(t):
    return None if t is None else t.data_ptr()


def _s():
    return torch.cuda.current_stream().cuda_stream


def _fn(name, dtype):
    from sid_lsg_amd._lib import lib
    if name == 'add':
        return lib.sidlsg_add_bf16 if dtype == BF16 else lib.sidlsg_add_f32
    return getattr(lib, f'sidlsg_{name}_f32' if dtype == F32 else f'sidlsg_{name}')


def _note(key, ratio):
    _worst[key] = max(_worst.get(key, 0.0), ratio)
    print(f'  {key}: {ratio:.3f} of the bound')
    return ratio


def _nm(dtype):
    return 'bf16' if dtype == BF16 else 'f32'


# ---- 1. activation value sweep -----------------------------------------------------------------------------------------------------
def _run_act(dev, op, x, a, dy, dtype, F=ec.SWEEP_F):
    """The op on flat x (GEGLU: as the gate half of h [n / F][2F]) -> outputs flat in x's order, guard zones checked."""
    n = x.numel()
    xd, dyd = x.to(dev), None if dy is None else dy.to(dev)
    nan_in = torch.isnan(x.double())             # NaN in gives NaN out, possibly with the payload of the sentinel
    if op == 'silu_fwd':
        y = ec.Guarded(n, dtype, dev)
        _fn('silu_fwd', dtype)(_p(xd), y.ptr(), n, _s())
        outs = [y]
    elif op == 'silu_bwd':
        y = ec.Guarded(n, dtype, dev)
        _fn('silu_bwd', dtype)(_p(xd), _p(dyd), y.ptr(), n, _s())
        outs = [y]
    else:
        M = n // F
        h = torch.cat([a.view(M, F), x.view(M, F)], 1).contiguous().to(dev)
        if op == 'geglu_fwd':
            y = ec.Guarded((M, F), dtype, dev)
            _fn('geglu_fwd', dtype)(_p(h), y.ptr(), M, F, _s())
            outs = [y]
        else:
            y = ec.Guarded((M, 2 * F), dtype, dev)
            before = h.clone()
            _fn('geglu_bwd', dtype)(_p(h), _p(dyd), y.ptr(), M, F, _s())
            torch.cuda.synchronize()
            assert ec.bits_equal(h, before)
            y.check(op, allow=torch.cat([nan_in.view(M, F)] * 2, 1))
            return [y.t[:, :F].cpu().flatten(), y.t[:, F:].cpu().flatten()]
    torch.cuda.synchronize()
    return [o.check(op, allow=nan_in).cpu().flatten() for o in outs]


@DTYPES
@pytest.mark.parametrize('op,variant', [(o, v) for o in ec.ACT_OPS for v in ec.ACT_VARIANTS if (o, v) != ('silu_fwd', 'randn')])
def test_activation_sweep(dev, op, variant, dtype):
    i = ec.sweep_inputs(op, variant, dtype)
    x = i['x']
    fin, nan_in = torch.isfinite(x.double()), torch.isnan(x.double())
    assert (~fin).sum().item() == 256
    got = _run_act(dev, op, x, i['a'], i['dy'], dtype)
    ref = ec.act_ref64(op, x, i['a'], i['dy'])
    for k, (g, r) in enumerate(zip(got, ref)):
        assert torch.isnan(g[nan_in].float()).all(), f'{op}: NaN in must give NaN out'
        ratio = _note(f'{op}{"_gate" if k else ""} {_nm(dtype)}', ec.act_ratio(g, r, dtype, ec.A_OF[dtype], fin))
        assert ratio <= 1.0, f'{op} {variant} output {k}: {ratio:.3g}x the bound ulp + A (bf16) / 2e-5 |ref| + A (fp32)'


# ---- 2. activation and layout shapes -----------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize('n', ec.SILU_N)
def test_silu_and_add_shapes(dev, n, dtype):
    x, dy = ec.randn_bf16(n, 1, 3.0).to(dtype), ec.randn_bf16(n, 2).to(dtype)
    for op in ('silu_fwd', 'silu_bwd'):
        got, = _run_act(dev, op, x, None, dy, dtype)
        ref, = ec.act_ref64(op, x, None, dy)
        assert _note(f'{op} shapes {_nm(dtype)}', ec.act_ratio(got, ref, dtype, ec.A_OF[dtype])) <= 1.0
    a, b = ec.int_values((n,), 3, dtype), ec.int_values((n,), 4, dtype)
    o = ec.Guarded(n, dtype, dev)
    ad, bd = a.to(dev), b.to(dev)
    _fn('add', dtype)(_p(ad), _p(bd), o.ptr(), n, _s())
    torch.cuda.synchronize()
    assert torch.equal(o.check('add').cpu().double(), a.double() + b.double())


@DTYPES
@pytest.mark.parametrize('M,F', ec.GEGLU_MF)
def test_geglu_shapes(dev, M, F, dtype):
    n = M * F
    x, a, dy = ec.randn_bf16(n, 5, 3.0).to(dtype), ec.randn_bf16(n, 6).to(dtype), ec.randn_bf16(n, 7).to(dtype)
    for op in ('geglu_fwd', 'geglu_bwd'):
        got = _run_act(dev, op, x, a, dy, dtype, F=F)
        ref = ec.act_ref64(op, x, a, dy)
        for g, r in zip(got, ref):
            assert _note(f'{op} shapes {_nm(dtype)}', ec.act_ratio(g, r, dtype, ec.A_OF[dtype])) <= 1.0


@DTYPES
@pytest.mark.parametrize('M,C1,C2', ec.CONCAT_CASES)
def test_concat2_both_directions(dev, M, C1, C2, dtype):
    a = ec.distinct_values(M * C1, dtype).view(M, C1)
    b = ec.distinct_values(M * C2, dtype, start=M * C1).view(M, C2)
    full = torch.cat([a, b], 1)
    fn = _fn('concat2', dtype)
    out = ec.Guarded((M, C1 + C2), dtype, dev)
    ad, bd = ec.Guarded((M, C1), dtype, dev, fill=a), ec.Guarded((M, C2), dtype, dev, fill=b)
    fn(ad.ptr(), bd.ptr(), out.ptr(), M, C1, C2, 0, _s())
    torch.cuda.synchronize()
    assert torch.equal(out.check('concat').cpu(), full) and ad.untouched() and bd.untouched()
    src = ec.Guarded((M, C1 + C2), dtype, dev, fill=full)
    pa, pb = ec.Guarded((M, C1), dtype, dev), ec.Guarded((M, C2), dtype, dev)
    fn(pa.ptr(), pb.ptr(), src.ptr(), M, C1, C2, 1, _s())
    torch.cuda.synchronize()
    assert torch.equal(pa.check('split a').cpu(), a) and torch.equal(pb.check('split b').cpu(), b)
    assert src.untouched(), 'the split changed its source'


@DTYPES
@pytest.mark.parametrize('B,H,W,C', ec.SUMPOOL_CASES)
def test_sumpool2x2_exact(dev, B, H, W, C, dtype):
    g = ec.int_values((B, 2 * H, 2 * W, C), 7 + H, dtype)
    out = ec.Guarded((B, H, W, C), dtype, dev)
    gd = g.to(dev)
    _fn('sumpool2x2', dtype)(_p(gd), out.ptr(), B, H, W, C, _s())
    torch.cuda.synchronize()
    assert torch.equal(out.check('sumpool2x2').cpu().double(), ec.sumpool_ref(g))


@DTYPES
@pytest.mark.parametrize('C', ec.ZERO_INSERT_C)
@pytest.mark.parametrize('H,W', ec.ZERO_INSERT_HW)
def test_zero_insert2_exact(dev, H, W, C, dtype):
    B, Ho, Wo = ec.ZERO_INSERT_B, (H + 1) // 2, (W + 1) // 2
    g = ec.int_values((B, Ho, Wo, C), 9 + H + W, dtype)
    out = ec.Guarded((B, H, W, C), dtype, dev)
    gd = g.to(dev)
    _fn('zero_insert2', dtype)(_p(gd), out.ptr(), B, Ho, Wo, H, W, C, _s())
    torch.cuda.synchronize()
    assert ec.bits_equal(out.check('zero_insert2').cpu(), ec.zero_insert_ref(g, H, W)), 'values, or an inserted zero that is not +0'


# ---- 3. colsum ---------------------------------------------------------------------------------------------------------------------
def _colsum_case(dev, dtype, B, rows, N, fill_ws):
    """Every (ldg, entry point, outputs) combination of one case in the current mode; exact."""
    from sid_lsg_amd import ops
    from sid_lsg_amd._lib import lib
    assert lib.sidlsg_colsum_nchunks.raw(B, rows) == ec.colsum_nchunks(B, rows)
    g = ec.int_values((B, rows, N), 40 + B + rows + N)
    ref_pb, ref_tot = ec.colsum_ref(g)
    ws = ops.ensure_workspace(dev)
    for ldg in (N, N + 16):
        gd = torch.full((B * rows, ldg), NAN, dtype=dtype, device=dev)      # the pad columns must never be read into a sum
        gd[:, :N] = g.view(-1, N).to(dtype).to(dev)
        for strided in (False, True):
            ld_pb = N + ec.COLSUM_LD_PB_EXTRA if strided else N
            sh = ec.COLSUM_PB_SHIFT if strided else 0
            for outputs in (('pb',), ('tot',), ('pb', 'tot')):
                pb_fill, tot_fill = ec.int_values((B, ld_pb), 3), ec.int_values((N,), 4)
                pb = ec.Guarded((B, ld_pb), F32, dev, fill=pb_fill) if 'pb' in outputs else None
                tot = ec.Guarded(N, F32, dev, fill=tot_fill) if 'tot' in outputs else None
                if fill_ws:     # scratch only (ops.ensure_workspace: torch.empty, nothing in it outlives a call): a slab cell that a
                    ws[:B * 128 * N + B * N + 64].fill_(NAN)     # chunk failed to write would reach the sums as NaN
                if strided:
                    _fn('colsum_strided', dtype)(_p(gd), ldg, None if pb is None else pb.ptr() + 4 * sh, ld_pb, None if tot is None else tot.ptr(),
                                                 B, rows, N, _s())
                else:
                    _fn('colsum', dtype)(_p(gd), ldg, None if pb is None else pb.ptr(), None if tot is None else tot.ptr(), None, B, rows, N, _s())
                torch.cuda.synchronize()
                what = f'colsum B{B} rows{rows} N{N} ldg{ldg} strided={strided} {outputs}'
                if pb is not None:
                    want = pb_fill.double()
                    want[:, sh:sh + N] += ref_pb
                    assert torch.equal(pb.check(what).cpu().double(), want), what + ': per_batch'
                if tot is not None:
                    assert torch.equal(tot.check(what).cpu().double(), tot_fill.double() + ref_tot), what + ': total'


@DTYPES
@pytest.mark.parametrize('B,rows,N', ec.COLSUM_CASES)
def test_colsum_exact(dev, mode, B, rows, N, dtype):
    _colsum_case(dev, dtype, B, rows, N, fill_ws=mode == 'det')


@pytest.mark.parametrize('B,rows,N', ec.COLSUM_NO_WS)
def test_colsum_exact_deterministic_without_workspace(dev, B, rows, N):
    from sid_lsg_amd import ops
    from sid_lsg_amd._lib import lib
    ws = ops.ensure_workspace(dev)
    old = ops._det_explicit
    ops.set_deterministic(True)
    lib.sidlsg_set_workspace(None, 0)
    try:
        _colsum_case(dev, BF16, B, rows, N, fill_ws=False)
    finally:
        torch.cuda.synchronize()
        lib.sidlsg_set_workspace(ws.data_ptr(), ws.numel() * 4)
        ops.set_deterministic(old)


# ---- 4. losses ---------------------------------------------------------------------------------------------------------------------
SCALE = 0.25


def _dropped(*ts):
    d = torch.zeros(ts[0].shape[0], dtype=torch.bool)
    for t in ts:
        d |= torch.isnan(t).flatten(1).any(1)
    return d


@pytest.mark.parametrize('c', ec.LOSS_CASES, ids=ec.loss_case_id)
def test_generator_loss_cases(dev, c):
    from oracle import sid_ref
    from sid_lsg_amd import ops
    from sid_lsg_amd._lib import lib
    i = ec.loss_inputs(c)
    x, yr, yf = i['x'], i['y_real'], i['y_fake']
    drop = _dropped(x, yr, yf)
    a, b, cc = (v.double().clone().requires_grad_() for v in (x, yr, yf))
    lref, _ = sid_ref.generator_loss_ref(a, b, cc, c.alpha, 1.0, 4)
    lref.backward()
    ad, bd, cd = (v.to(dev).requires_grad_() for v in (x, yr, yf))
    loss = ops.sid_generator_loss(ad, bd, cd, c.alpha, SCALE)
    loss.backward()
    torch.cuda.synchronize()
    r = _note('g_loss', ec.loss_ratio(loss.detach(), lref.detach(), (ad.grad, bd.grad, cd.grad), (a.grad, b.grad, cc.grad), drop))
    assert r <= 1.0, f'{r:.3g}x the bound (value 1e-5 relative, gradients 1e-5 of the maximum in each sample, dropped samples exactly 0)'
    if drop.all():
        assert float(loss) == 0.0
    # the same launch into guarded buffers: bit-equal, nothing outside the extents
    S, n = c.S, x[0].numel()
    outs = [ec.Guarded(x.shape, F32, dev) for _ in range(3)]
    lg, ws = ec.Guarded(1, F32, dev), ec.Guarded(10 * S, F32, dev)
    lib.sidlsg_g_loss(_p(ad.detach()), _p(bd.detach()), _p(cd.detach()), outs[0].ptr(), outs[1].ptr(), outs[2].ptr(), lg.ptr(), ws.ptr(), S, n,
                      float(c.alpha), SCALE, _s())
    torch.cuda.synchronize()
    for o, gr in zip(outs, (ad.grad, bd.grad, cd.grad)):
        assert ec.bits_equal(o.check('g_loss gradient'), gr)
    assert ec.bits_equal(lg.check('g_loss value'), loss.detach().view(1))
    ws.check('g_loss workspace')


@pytest.mark.parametrize('c', ec.LOSS_CASES, ids=ec.loss_case_id)
def test_fake_score_loss_cases(dev, c):
    from oracle import sid_ref
    from sid_lsg_amd import ops
    i = ec.loss_inputs(c)
    e, noise = i['x'], torch.nan_to_num(i['y_real'])
    drop = _dropped(e)
    er = e.double().clone().requires_grad_()
    lref, _ = sid_ref.fake_score_loss_ref(er, noise.double(), 1.0, 4)
    lref.backward()
    ed = e.to(dev).requires_grad_()
    loss = ops.sid_fake_score_loss(ed, noise.to(dev), SCALE)
    loss.backward()
    torch.cuda.synchronize()
    r = _note('fake_loss', ec.loss_ratio(loss.detach(), lref.detach(), (ed.grad,), (er.grad,), drop))
    assert r <= 1.0
    # the v form: a NaN in the images or the noise drops the sample as well
    o, images, nz = i['x'], i['y_real'], i['y_fake']
    vref, gref, vdrop = ec.fake_loss_v_ref64(o, images, nz, i['s0'], i['s1'], i['w'], SCALE)
    assert torch.equal(vdrop, _dropped(o, images, nz))
    od = o.to(dev).requires_grad_()
    vloss = ops.sid_fake_score_loss_v(od, images.to(dev), nz.to(dev), i['s0'].to(dev), i['s1'].to(dev), i['w'].to(dev), SCALE)
    vloss.backward()
    torch.cuda.synchronize()
    r = _note('fake_loss_v', ec.loss_ratio(vloss.detach(), vref, (od.grad,), (gref,), vdrop))
    assert r <= 1.0


# ---- 5. optimizer ------------------------------------------------------------------------------------------------------------------
def _make_opt(dev, cfg, n, p0):
    from sid_lsg_amd.optim import FusedAdamEMA, FusedAdamWEMA
    b = dict(p=ec.Guarded(n, F32, dev, fill=p0), g=ec.Guarded(n, F32, dev, fill=0.0), ema=ec.Guarded(n, F32, dev, fill=p0),
             w16=ec.Guarded(n, BF16, dev), v=ec.Guarded(n, F32, dev, fill=0.0))
    cls = FusedAdamWEMA if cfg.decoupled else FusedAdamEMA
    opt = cls.from_flat(b['p'].t, b['g'].t, lr=cfg.lr, betas=cfg.betas, eps=cfg.eps, weight_decay=cfg.weight_decay, decoupled=cfg.decoupled,
                        clip_value=cfg.clip, ema=b['ema'].t, w16=b['w16'].t)
    opt.grad_scale = cfg.grad_scale
    opt.exp_avg_sq = b['v'].t
    if opt.exp_avg is not None:
        b['m'] = ec.Guarded(n, F32, dev, fill=0.0)
        opt.exp_avg = b['m'].t
    return opt, b


@pytest.mark.parametrize('n', ec.ADAM_N)
@pytest.mark.parametrize('cfg', ec.ADAM_CFGS, ids=lambda c: c.name)
def test_adam_ema_cases(dev, cfg, n):
    from oracle import sid_ref
    p0 = torch.randn(n, generator=torch.Generator().manual_seed(1))
    opt, b = _make_opt(dev, cfg, n, p0)
    p_ref, ema_ref, st = p0.clone(), p0.clone(), {}
    tp = topt = None
    if n <= 1027 and cfg.weight_decay:
        tp = torch.nn.Parameter(p0.clone())
        topt = (torch.optim.AdamW if cfg.decoupled else torch.optim.Adam)([tp], lr=cfg.lr, betas=cfg.betas, eps=cfg.eps, weight_decay=cfg.weight_decay)
    for step in range(ec.adam_steps(n)):
        gr, beta = ec.adam_grad(n, step), ec.adam_beta(n, step)
        b['g'].t.copy_(gr)
        keep = step == ec.ADAM_KEEP_GRAD_STEP
        opt.step(ema_beta=beta, zero_grad=not keep)
        torch.cuda.synchronize()
        if keep:
            assert ec.bits_equal(b['g'].t.cpu(), gr), 'zero_grad=False must leave the gradient buffer bit-unchanged'
        else:
            assert not b['g'].t.view(torch.int32).any(), 'zero_grad folded into the step'
        sid_ref.adam_step_ref(p_ref, gr * cfg.grad_scale, st, cfg.lr, cfg.betas, cfg.eps, cfg.weight_decay, cfg.decoupled, cfg.clip)
        sid_ref.ema_update_ref(ema_ref, p_ref, beta)
        refs = dict(p=p_ref, ema=ema_ref, v=st['exp_avg_sq'])
        if 'm' in b:
            refs['m'] = st['exp_avg']
        for k, r in refs.items():
            ratio = _note(f'adam {k}', ec.adam_ratio(b[k].t, r, n))
            assert ratio <= 1.0, f'{cfg.name} n={n} step {step}: {k} at {ratio:.3g}x the bound of 1e-6 of the maximum'
        if topt is not None:
            gg = torch.nan_to_num(gr * cfg.grad_scale, nan=0.0, posinf=1e5, neginf=-1e5)
            tp.grad = gg.clamp(-cfg.clip, cfg.clip) if cfg.clip is not None else gg
            topt.step()
            assert _note('adam p vs torch.optim', ec.adam_ratio(b['p'].t, tp.detach(), n, ec.ADAM_TOL_TORCH)) <= 1.0
        assert ec.bits_equal(b['w16'].t, b['p'].t.to(BF16)), 'bf16 compute copy = RNE(bf16) of the updated master'
        for k, gd in b.items():
            gd.check(f'adam {k}')


@pytest.mark.parametrize('n', [1027, ec.ADAM_LARGE])
def test_adam_launch_range_partition_is_bit_equal(dev, n):
    cfg = ec.ADAM_CFGS[1]
    p0 = torch.randn(n, generator=torch.Generator().manual_seed(2))
    whole, bw = _make_opt(dev, cfg, n, p0)
    parts, bp = _make_opt(dev, cfg, n, p0)
    cuts = [0, 4, 256, 1000, n] if n == 1027 else [0, 4, 4194304, 4194304 + 1200, n]
    assert all(c % 4 == 0 for c in cuts[:-1]) and n % 4
    for step in range(2):
        gr, beta = ec.adam_grad(n, step), ec.adam_beta(n, step)
        bw['g'].t.copy_(gr)
        bp['g'].t.copy_(gr)
        whole.step(ema_beta=beta)
        parts.begin_step(beta)
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            parts.launch_range(lo, hi, use_ema=True, zero_grad=True)
        torch.cuda.synchronize()
        for k in bw:
            assert torch.equal(bw[k].bits(), bp[k].bits()), f'{k}: the partitioned launch differs from the single one (step {step})'
            bp[k].check(k)


# ---- 6. weight preparation ---------------------------------------------------------------------------------------------------------
def test_cast_f32_bf16_every_pattern(dev):
    from sid_lsg_amd._lib import lib
    x = ec.cast_words()
    y = ec.Guarded(x.numel(), BF16, dev)
    xd = x.to(dev)
    lib.sidlsg_cast_f32_bf16(_p(xd), y.ptr(), x.numel(), _s())
    torch.cuda.synchronize()
    got, ref = y.check('cast', allow=torch.isnan(x)).cpu(), ec.cast_ref(x)
    bad = ~((got.view(torch.int16) == ref.view(torch.int16)) | (torch.isnan(got) & torch.isnan(ref)))
    assert ec.cast_equal(got, ref), f'{int(bad.sum())} words differ from round-to-nearest-even, first: {x.view(torch.int32)[bad][:4].tolist()}'


@pytest.mark.parametrize('n', ec.CAST_N)
def test_cast_f32_bf16_tails(dev, n):
    from sid_lsg_amd._lib import lib
    x = torch.randn(n, generator=torch.Generator().manual_seed(n))
    y = ec.Guarded(n, BF16, dev)
    xd = x.to(dev)
    lib.sidlsg_cast_f32_bf16(_p(xd), y.ptr(), n, _s())
    torch.cuda.synchronize()
    assert ec.bits_equal(y.check('cast').cpu(), ec.cast_ref(x))


@pytest.mark.parametrize('ns', ec.SCALE_CAST_TABLES, ids=lambda ns: f'{len(ns)}jobs')
def test_scale_cast_ranges(dev, ns):
    import numpy as np
    from sid_lsg_amd._lib import lib
    scales = [40 ** -0.5 * 1.4426950408889634, 1.0, -3.0, 0.125, 64 ** -0.5 * 1.4426950408889634]
    jobs, keep = [], []
    for j, n in enumerate(ns):
        src = torch.randn(n, generator=torch.Generator().manual_seed(50 + n))
        hold = torch.zeros(n + 8, device=dev)
        s_sh = 1 if j == 0 else 0                                  # one float past 16-byte alignment
        sd = hold[s_sh:s_sh + n]
        sd.copy_(src)
        dst = ec.Guarded(n, BF16, dev, shift=1 if j == len(ns) - 1 else 0)      # one bf16 past it
        assert sd.data_ptr() % 16 == 4 * s_sh and dst.ptr() % 16 == (2 if j == len(ns) - 1 else 0)
        jobs.append((sd.data_ptr(), dst.ptr(), n, scales[j]))
        keep.append((src, dst, scales[j], hold))
    tab, nj, nb = ec.sc_table(jobs)
    tabd = tab.to(dev)
    lib.sidlsg_scale_cast_ranges(_p(tabd), nj, nb, _s())
    torch.cuda.synchronize()
    for src, dst, scale, _ in keep:
        assert ec.bits_equal(dst.check('scale_cast_ranges').cpu(), (src * float(np.float32(scale))).to(BF16)), f'n = {src.numel()}'


def _transpose_jobs(dev, table, kind):
    """kind 'bf16' / 'f32': fp32 sources to that destination type; 'w16': bf16 sources to bf16."""
    dst_dtype = F32 if kind == 'f32' else BF16
    recs, keep = [], []
    for N, K, T in table:
        src = ec.finite_bf16(N * T * K, N + K + T)
        sd = (src if kind == 'w16' else src.float()).to(dev)
        dst = ec.Guarded((K, T, N), dst_dtype, dev)
        recs.append((sd.data_ptr(), dst.ptr(), N, K, T))
        keep.append((sd, dst, ec.transpose_ref(src.to(dst_dtype), N, K, T)))
    return recs, keep


@pytest.mark.parametrize('kind', ['bf16', 'f32', 'w16'])
def test_transpose_w_batched_tables(dev, kind):
    from sid_lsg_amd._lib import lib
    for table in (ec.TRANSPOSE_TABLES if kind == 'w16' else ec.TRANSPOSE_TABLES_F32):
        recs, keep = _transpose_jobs(dev, table, kind)
        tab, nj, nb = ec.tw_table(recs, 64 if kind == 'w16' else 32)
        fn = lib.sidlsg_transpose_w16_batched if kind == 'w16' else _fn('transpose_w_batched', F32 if kind == 'f32' else BF16)
        tabd = tab.to(dev)
        fn(_p(tabd), nj, nb, _s())
        torch.cuda.synchronize()
        for (N, K, T), (_, dst, ref) in zip(table, keep):
            assert torch.equal(dst.check(f'transpose {kind} {N, K, T}').cpu(), ref), f'{kind} {N, K, T} in a table of {nj}'


@DTYPES
@pytest.mark.parametrize('N,K,T', ec.TRANSPOSE_CASES + ec.TRANSPOSE_F32_ONLY)
def test_transpose_w_single(dev, N, K, T, dtype):
    recs, keep = _transpose_jobs(dev, ((N, K, T),), 'f32' if dtype == F32 else 'bf16')
    sd, dst, ref = keep[0]
    _fn('transpose_w', dtype)(_p(sd), dst.ptr(), N, K, T, _s())
    torch.cuda.synchronize()
    assert torch.equal(dst.check('transpose_w').cpu(), ref)


# ---- 7. timestep embedding ---------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize('dim', ec.TEMB_DIMS)
def test_timestep_embedding(dev, dim, dtype):
    t = torch.tensor(ec.TEMB_T, dtype=torch.int64)
    out = ec.Guarded((len(ec.TEMB_T), dim), dtype, dev)
    td = t.to(dev)
    _fn('timestep_embed', dtype)(_p(td), out.ptr(), len(ec.TEMB_T), dim, _s())
    torch.cuda.synchronize()
    r = _note(f'timestep_embed {_nm(dtype)}', ec.max_rel(out.check('timestep_embed'), ec.timestep_ref64(t, dim)) / ec.TEMB_TOL[dtype])
    assert r <= 1.0


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_launchers_refuse_bad_arguments(dev, dtype):
    """Every argument check of the launchers returns SIDLSG_EINVAL and writes nothing.  (The sizes are such that even a launcher
    without the check would stay inside these buffers.)"""
    f = lambda: torch.ones(1024, device=dev)                                          # noqa: E731
    act = lambda: torch.ones(1024, device=dev, dtype=dtype)                           # noqa: E731
    out, fout = ec.Guarded(1024, dtype, dev), ec.Guarded(1024, F32, dev)
    s, one = _s(), torch.ones(4, device=dev)
    R = lambda name, *a: _fn(name, dtype).raw(*a)                                     # noqa: E731
    calls = {
        'noisy_input C > 8': R('noisy_input', _p(f()), _p(f()), _p(one), _p(one), out.ptr(), fout.ptr(), 1, 9, 4, 16, 1, s),
        'noisy_input Cp % 8': R('noisy_input', _p(f()), _p(f()), _p(one), _p(one), out.ptr(), fout.ptr(), 1, 4, 4, 12, 1, s),
        'noisy_input_bwd C > 8': R('noisy_input_bwd', _p(act()), _p(one), fout.ptr(), 1, 9, 4, 16, 1, 0, s),
        'noisy_input_bwd Cp % 8': R('noisy_input_bwd', _p(act()), _p(one), fout.ptr(), 1, 4, 4, 12, 1, 0, s),
        'noisy_input_bwd Cp < 8': R('noisy_input_bwd', _p(act()), _p(one), fout.ptr(), 1, 4, 4, 0, 1, 0, s),
        'cfg_x0_bwd C > 8': R('cfg_x0_bwd', _p(f()), _p(one), _p(one), out.ptr(), fout.ptr(), 1, 9, 4, 16, 1, 1.5, 1, s),
        'cfg_x0_bwd Cp % 8': R('cfg_x0_bwd', _p(f()), _p(one), _p(one), out.ptr(), fout.ptr(), 1, 4, 4, 12, 1, 1.5, 1, s),
        'cfg_x0_bwd Cp < 8': R('cfg_x0_bwd', _p(f()), _p(one), _p(one), out.ptr(), fout.ptr(), 1, 4, 4, 0, 1, 1.5, 1, s),
        'silu_fwd n % 8': R('silu_fwd', _p(act()), out.ptr(), 12, s),
        'silu_bwd n % 8': R('silu_bwd', _p(act()), _p(act()), out.ptr(), 12, s),
        'add n % 8': R('add', _p(act()), _p(act()), out.ptr(), 12, s),
        'geglu_fwd F % 8': R('geglu_fwd', _p(act()), out.ptr(), 2, 12, s),
        'geglu_bwd F % 8': R('geglu_bwd', _p(act()), _p(act()), out.ptr(), 2, 12, s),
        'concat2 C1 % 8': R('concat2', _p(act()), _p(act()), out.ptr(), 2, 12, 8, 0, s),
        'concat2 C2 % 8': R('concat2', _p(act()), _p(act()), out.ptr(), 2, 8, 12, 0, s),
        'sumpool2x2 C % 8': R('sumpool2x2', _p(act()), out.ptr(), 1, 2, 2, 12, s),
        'zero_insert2 C % 8': R('zero_insert2', _p(act()), out.ptr(), 1, 2, 2, 4, 4, 12, s),
        'zero_insert2 H != 2 Ho, 2 Ho - 1': R('zero_insert2', _p(act()), out.ptr(), 1, 2, 2, 6, 4, 8, s),
        'zero_insert2 W != 2 Wo, 2 Wo - 1': R('zero_insert2', _p(act()), out.ptr(), 1, 2, 2, 4, 2, 8, s),
        'colsum N % 8': R('colsum', _p(act()), 16, fout.ptr(), fout.ptr(), None, 2, 4, 12, s),
        'colsum N = 0': R('colsum', _p(act()), 16, fout.ptr(), fout.ptr(), None, 2, 4, 0, s),
        'colsum_strided ld_pb < N': R('colsum_strided', _p(act()), 16, fout.ptr(), 8, fout.ptr(), 2, 4, 16, s),
    }
    torch.cuda.synchronize()
    for what, rc in calls.items():
        assert rc == ec.EINVAL, f'{what}: returned {rc}, not SIDLSG_EINVAL'
    assert out.untouched() and fout.untouched(), 'a refused call wrote to its output'


def test_losses_and_optimizer_refuse_bad_arguments(dev):
    from sid_lsg_amd._lib import lib
    f = lambda: torch.ones(64, device=dev)                                            # noqa: E731
    outs = [ec.Guarded(64, F32, dev) for _ in range(5)]
    o = [g.ptr() for g in outs]
    s = _s()
    for S, n in ((0, 8), (2, 0), (-1, 8), (2, -8)):
        assert lib.sidlsg_g_loss.raw(_p(f()), _p(f()), _p(f()), o[0], o[1], o[2], o[3], o[4], S, n, 1.0, 1.0, s) == ec.EINVAL
        assert lib.sidlsg_fake_loss.raw(_p(f()), _p(f()), o[0], o[3], o[4], S, n, 1.0, s) == ec.EINVAL
        assert lib.sidlsg_fake_loss_v.raw(_p(f()), _p(f()), _p(f()), _p(f()), _p(f()), _p(f()), o[0], o[3], o[4], S, n, 1.0, s) == ec.EINVAL
    # the optimizer: 16-byte vector accesses on p, g, v
    p, g, v, hyper = (ec.Guarded(64, F32, dev, fill=1.0) for _ in range(4))
    for k in range(3):
        ptrs = [p.ptr(), g.ptr(), v.ptr()]
        ptrs[k] += 4
        assert lib.sidlsg_adam_ema.raw(ptrs[0], ptrs[1], None, ptrs[2], None, None, hyper.ptr(), 8, 1, s) == ec.EINVAL
    assert lib.sidlsg_adam_ema.raw(p.ptr(), g.ptr(), None, v.ptr(), None, None, hyper.ptr(), 0, 1, s) == ec.EINVAL
    assert lib.sidlsg_adam_ema.raw(None, g.ptr(), None, v.ptr(), None, None, hyper.ptr(), 8, 1, s) == ec.EINVAL
    opt, b = _make_opt(dev, ec.ADAM_CFGS[0], 64, torch.ones(64))
    opt.begin_step(0.5)
    with pytest.raises(ValueError):
        opt.launch_range(2, 64)
    torch.cuda.synchronize()
    for gd in outs + [p, g, v, hyper] + list(b.values()):
        assert gd.untouched(), 'a refused call wrote to a buffer'
