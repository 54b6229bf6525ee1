"""The cases of tests/test_gpu_elementwise_edges.py (tests/elementwise_cases.py) checked on the CPU:

  * the bounds can be met: the fp32 emulations of the kernels' formulas, rounded to the storage type, stay inside the activation
    bounds; A_BF16 / A_F32 are what the module says they are (twice the measured absolute error, floor 1e-6); the fp32 CPU oracle of
    the losses and of the optimizer stays inside the bounds against fp64;
  * the exact checks are exact: every integer case keeps its partial sums below 2^24 and its values exact in bf16;
  * at most 0.5 % of a sweep is left out of the numeric comparison;
  * colsum_nchunks restated in Python yields an empty last chunk for rows = 8193;
  * the GPU tests can fail: every reference of MUTATIONS misses its family's bound by more than 10x, or its exact check, on at
    least one case of the table;
  * the guard-zone helper sees a write outside the extent and an element that was never written.

`pytest -s` prints every figure.
"""
import numpy as np
import pytest
import torch

import elementwise_cases as ec

BF16, F32, F64 = ec.BF16, ec.F32, ec.F64


# ---- activations -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [BF16, F32], ids=['bf16', 'f32'])
def test_activation_emulation_inside_bounds_and_constants_derived(dtype):
    A = ec.A_OF[dtype]
    worst_a = 0.0
    for op in ec.ACT_OPS:
        for variant in ec.ACT_VARIANTS:
            i = ec.sweep_inputs(op, variant, dtype)
            fin = torch.isfinite(i['x'].double())
            assert i['x'].numel() == (65536 if dtype == BF16 else 131072)
            assert (~fin).sum().item() == 256 and (~fin).float().mean().item() <= ec.NONFINITE_CAP
            ref = ec.act_ref64(op, i['x'], i['a'], i['dy'])
            emu = ec.act_emulated(op, i['x'], i['a'], i['dy'], dtype)
            for e, r in zip(emu, ref):
                ratio = ec.act_ratio(ec.store(e, dtype), r, dtype, A, fin)
                worst_a = max(worst_a, ec.act_excess(e[fin], r[fin], dtype))
                print(f'  {op} {variant}: emulation at {ratio:.3f} of the bound')
                assert ratio <= 1.0, f'{op} {variant}: the emulation misses the bound ({ratio:.3g}x)'
                nan_in = torch.isnan(i['x'].double())
                assert torch.isnan(e[nan_in]).all()
    derived = max(2 * worst_a, ec.A_FLOOR)
    print(f'  largest a {worst_a:.3e} -> A = {derived:.3e}, module: {A:.3e}')
    assert derived <= A <= 1.25 * derived, f'A = {A} but the measurement gives {derived}'


def test_sweep_mixes_nonfinite_inputs_with_finite_ones():
    for dtype in (BF16, F32):
        x = ec.sweep_x(dtype).double().view(-1, 8)
        bad = ~torch.isfinite(x)
        assert (bad.any(1) & ~bad.all(1)).sum().item() >= 200          # 8-vectors with a non-finite input and finite neighbours
    assert ec.sweep_x(BF16).view(torch.int16).unique().numel() == 65536


def test_ulp_bf16():
    v = torch.tensor([1.0, 1.5, 2.0, 0.0, 2.0 ** -126, 2.0 ** -127, 3.0e38, -0.75], dtype=F64)
    want = torch.tensor([2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -133, 2.0 ** -133, 2.0 ** -133, 2.0 ** 120, 2.0 ** -8], dtype=F64)
    assert torch.equal(ec.ulp_bf16(v), want)
    for x in (1.0, 0.0078125, 3.0e38):        # the spacing torch's own bf16 has there
        b = torch.tensor(x, dtype=BF16)
        nxt = (b.view(torch.int16) + 1).view(BF16)
        assert float(nxt.double() - b.double()) == float(ec.ulp_bf16(b.double()))


@pytest.mark.parametrize('mutation', ec.MUTATIONS['activations'])
def test_activation_mutations_miss(mutation):
    worst = 0.0
    for dtype in (BF16, F32):
        for op in ec.ACT_OPS:
            i = ec.sweep_inputs(op, 'ones', dtype)
            fin = torch.isfinite(i['x'].double())
            ref = ec.act_ref64(op, i['x'], i['a'], i['dy'])
            bad = ec.act_ref64(op, i['x'], i['a'], i['dy'], mutation=mutation)
            r = max(ec.act_ratio(ec.store(b.float(), dtype), r_, dtype, ec.A_OF[dtype], fin) for b, r_ in zip(bad, ref))
            print(f'  {mutation} {op} {dtype}: {r:.1f}x the bound')
            if dtype == BF16:
                worst = max(worst, r)
    assert worst > 10, f'{mutation}: at most {worst:.1f}x the bf16 bound: the GPU test could miss this bug'


# ---- exact integer cases -----------------------------------------------------------------------------------------------------------
def _colsum_input(B, rows, N, dtype=F32):
    return ec.int_values((B, rows, N), 40 + B + rows + N, dtype)


@pytest.mark.parametrize('B,rows,N', ec.COLSUM_CASES)
def test_colsum_case_is_exact(B, rows, N):
    g = _colsum_input(B, rows, N)
    assert g.abs().min() >= 1 and g.abs().max() <= 8
    assert torch.equal(g.to(BF16).float(), g)
    assert (g.abs().double().sum((0, 1)).max().item() + 8) < 2 ** 24           # any partial sum, the pre-fill included
    pb, tot = ec.colsum_ref(g)
    assert torch.equal(pb.float().double(), pb) and torch.equal(tot.float().double(), tot)
    # the chunks the kernel walks cover every row once
    ch = ec.colsum_chunks(B, rows)
    covered = [r for r0, r1 in ch for r in range(r0, r1)]
    assert covered == list(range(rows))


def test_colsum_chunking_has_an_empty_last_chunk():
    ch = ec.colsum_chunks(1, 8193)
    assert ec.colsum_nchunks(1, 8193) == 128 and len(ch) == 128
    assert ch[0] == (0, 65) and ch[126] == (8190, 8193)
    assert ch[127][0] > 8193 and ch[127][1] < ch[127][0]                       # starts past the last row
    assert ec.colsum_nchunks(5, 700) == 11 and ec.colsum_nchunks(1, 1) == 1 and ec.colsum_nchunks(16, 4096) == 32


@pytest.mark.parametrize('mutation', ec.MUTATIONS['colsum'])
def test_colsum_mutations_miss(mutation):
    missed = []
    for B, rows, N in ec.COLSUM_CASES:
        g = _colsum_input(B, rows, N)
        pb, tot = ec.colsum_ref(g)
        bpb, btot = ec.colsum_ref(g, mutation)
        if not torch.equal(pb, bpb) and not torch.equal(tot, btot):
            missed.append((B, rows, N))
    print(f'  {mutation}: unequal on {missed}')
    assert missed


def test_sumpool_and_zero_insert_cases():
    hit = False
    for B, H, W, C in ec.SUMPOOL_CASES:
        g = ec.int_values((B, 2 * H, 2 * W, C), 7 + H)
        ref = ec.sumpool_ref(g)
        assert torch.equal(ref.to(BF16).double(), ref) and ref.abs().max() <= 32
        assert not torch.equal(ec.sumpool_ref(g, 'tap_missing'), ref)
    for H, W in ec.ZERO_INSERT_HW:
        for C in ec.ZERO_INSERT_C:
            g = ec.int_values((ec.ZERO_INSERT_B, (H + 1) // 2, (W + 1) // 2, C), 9 + H + W)
            ref = ec.zero_insert_ref(g, H, W)
            assert ref.shape == (ec.ZERO_INSERT_B, H, W, C) and int((ref != 0).sum()) == g.numel()
            assert not torch.signbit(ref[ref == 0]).any()
            bad = ec.zero_insert_ref(g, H, W, 'odd_as_even')
            assert torch.equal(bad, ref) == (H % 2 == 0 and W % 2 == 0) or (H, W) == (1, 1)
            hit |= not torch.equal(bad, ref)
    assert hit
    assert {(h % 2, w % 2) for h, w in ec.ZERO_INSERT_HW} == {(1, 1), (1, 0), (0, 1)} and {((h + 1) // 2) % 2 for h, _ in ec.ZERO_INSERT_HW} == {0, 1}


# ---- losses ------------------------------------------------------------------------------------------------------------------------
def _sid_ref_g(i, alpha, dtype):
    from oracle import sid_ref
    a, b, c = (i[k].to(dtype).clone().requires_grad_() for k in ('x', 'y_real', 'y_fake'))
    loss, _ = sid_ref.generator_loss_ref(a, b, c, alpha, 1.0, 4)
    loss.backward()
    return loss.detach(), [t.grad for t in (a, b, c)]


def test_loss_table_covers_what_it_should():
    S = {c.S for c in ec.LOSS_CASES}
    n = {int(np.prod(c.shape)) for c in ec.LOSS_CASES}
    assert S == {1, 3, 9} and n == {1, 255, 2048, 2049, 4356}
    assert any(c.S == 9 and int(np.prod(c.shape)) == 4356 for c in ec.LOSS_CASES)
    assert {c.alpha for c in ec.LOSS_CASES} == {1.0, 1.2}
    where = {t for c in ec.LOSS_CASES for t, _, _ in c.nans}
    assert where == {'x', 'y_real', 'y_fake'}
    idx = {i for c in ec.LOSS_CASES for _, _, i in c.nans}
    assert idx >= {0, 64, 255, -1}
    assert any(len({s for _, s, _ in c.nans}) == 2 and c.S > 2 for c in ec.LOSS_CASES)             # two dropped
    assert sum(len({s for _, s, _ in c.nans}) == c.S for c in ec.LOSS_CASES) >= 2                  # every sample dropped
    assert any(c.clip is not None for c in ec.LOSS_CASES)
    assert len({ec.loss_case_id(c) for c in ec.LOSS_CASES}) == len(ec.LOSS_CASES)


@pytest.mark.parametrize('c', ec.LOSS_CASES, ids=ec.loss_case_id)
def test_loss_case(c):
    i = ec.loss_inputs(c)
    loss, dx, dyr, dyf, drop = ec.g_loss_ref64(i['x'], i['y_real'], i['y_fake'], c.alpha, 0.25)
    assert drop.tolist() == [s in {s_ for _, s_, _ in c.nans} for s in range(c.S)]
    # the closed form is the oracle: oracle/sid_ref.py in fp64 through autograd
    lref, gref = _sid_ref_g(i, c.alpha, F64)
    assert abs(float(loss) - float(lref)) <= 1e-12 * abs(float(lref)) + 1e-300
    for mine, theirs in zip((dx, dyr, dyf), gref):
        keep = ~drop
        assert torch.allclose(mine[keep], theirs[keep], rtol=1e-10, atol=0)
        assert float(theirs[drop].abs().sum()) == 0 if drop.any() else True
    if c.clip is not None:
        assert float((i['x'][c.clip] - i['y_real'][c.clip]).abs().max()) == 0        # w reaches the clip
    # the bound can be met: the same oracle in fp32
    l32, g32 = _sid_ref_g(i, c.alpha, F32)
    r = ec.loss_ratio(l32, lref, g32, gref, drop)
    print(f'  fp32 oracle at {r:.3f} of the bound')
    assert r <= 1.0


@pytest.mark.parametrize('mutation', ec.MUTATIONS['g_loss'])
def test_loss_mutations_miss(mutation):
    worst = 0.0
    for c in ec.LOSS_CASES:
        i = ec.loss_inputs(c)
        loss, dx, dyr, dyf, drop = ec.g_loss_ref64(i['x'], i['y_real'], i['y_fake'], c.alpha, 0.25)
        bl, bx, br, bf, _ = ec.g_loss_ref64(i['x'], i['y_real'], i['y_fake'], c.alpha, 0.25, mutation)
        worst = max(worst, ec.loss_ratio(bl, loss, (bx, br, bf), (dx, dyr, dyf), drop))
    print(f'  {mutation}: {worst:.3g}x the bound')
    assert worst > 10


# ---- optimizer ---------------------------------------------------------------------------------------------------------------------
def _run_adam(cfg, n, dtype, mutation=None, use_sid_ref=False):
    from oracle import sid_ref
    p = torch.randn(n, generator=torch.Generator().manual_seed(1)).to(dtype)
    ema, st, hist = p.clone(), {}, []
    for step in range(ec.adam_steps(n)):
        g, beta = ec.adam_grad(n, step).to(dtype), ec.adam_beta(n, step)
        if use_sid_ref:
            sid_ref.adam_step_ref(p, g * cfg.grad_scale, st, cfg.lr, cfg.betas, cfg.eps, cfg.weight_decay, cfg.decoupled, cfg.clip)
            sid_ref.ema_update_ref(ema, p, beta)
            m, v = st['exp_avg'], st['exp_avg_sq']
        else:
            ec.adam_ema_ref(p, g, ema, st, cfg, beta, mutation)
            m, v = st['m'], st['v']
        hist.append(dict(p=p.clone(), ema=ema.clone(), m=m.clone(), v=v.clone()))
    return hist


@pytest.mark.parametrize('cfg', ec.ADAM_CFGS, ids=lambda c: c.name)
def test_adam_reference_and_mutations(cfg):
    n = 1027
    sp = ec.adam_special(n)
    assert sp[:3] == [0, 1, 2] and sp[3:] == [1024, 1025, 1026]
    assert ec.adam_special(3) == [0, 1, 2] and ec.adam_special(4) == [0, 1, 2] and ec.adam_special(5) == [0, 1, 2, 4]
    assert ec.adam_special(ec.ADAM_LARGE)[-3:] == [ec.ADAM_LARGE - 3, ec.ADAM_LARGE - 2, ec.ADAM_LARGE - 1]
    kinds = set()
    for step in range(5):
        g = ec.adam_grad(n, step)
        kinds |= {('nan' if v != v else v) for v in g[[1024, 1025, 1026]].tolist()}
    assert kinds == {'nan', float('inf'), -float('inf')}
    ref = _run_adam(cfg, n, F64)
    oracle = _run_adam(cfg, n, F64, use_sid_ref=True)
    for a, b in zip(ref, oracle):
        for k in 'p ema m v'.split():
            assert torch.allclose(a[k], b[k], rtol=1e-12, atol=0), k
    f32 = _run_adam(cfg, n, F32)          # the bound can be met: fp32 against fp64
    worst = max(ec.adam_ratio(a[k], b[k], n) for a, b in zip(f32, ref) for k in 'p ema m v'.split())
    print(f'  fp32 reference at {worst:.3f} of the bound')
    assert worst <= 1.0
    for mutation in ec.MUTATIONS['adam']:
        if mutation == 'decay_swapped' and cfg.weight_decay == 0:
            continue
        if mutation == 'eps_inside_root' and cfg.name != 'recipe':
            continue                       # eps shows where the gradient is tiny: no decay, no first moment
        bad = _run_adam(cfg, n, F64, mutation)
        r = max(ec.adam_ratio(a[k], b[k], n) for a, b in zip(bad, ref) for k in ('p', 'ema'))
        print(f'  {cfg.name} {mutation}: {r:.3g}x the bound')
        assert r > 10, mutation


def test_adam_table_covers_both_ema_forms_and_the_second_pass():
    assert {b < 0.5 for b in ec.ADAM_BETAS} == {True, False} and 0.5 in ec.ADAM_BETAS
    assert ec.ADAM_LARGE > 4096 * 256 * 4 and (ec.ADAM_LARGE - 4096 * 256 * 4) % 4 == 3
    assert set(ec.ADAM_N) >= {1, 3, 4, 5, 1027}


# ---- weight preparation ------------------------------------------------------------------------------------------------------------
def test_cast_cases():
    w = ec.cast_words()
    assert w.numel() == 65536 * 6 and w.view(torch.int32).unique().numel() == 65536 * 6
    ref = ec.cast_ref(w)
    assert ec.cast_equal(ref, ref.clone())
    bad = ec.cast_ref(w, 'truncation')
    assert not ec.cast_equal(bad, ref)
    # a NaN whose upper half is the pattern of infinity: truncation returns inf
    i = (0x7f80 * 6) + 1
    assert torch.isnan(w[i]) and torch.isnan(ref[i]) and torch.isinf(bad[i].float())


def test_transpose_cases():
    for N, K, T in ec.TRANSPOSE_CASES + ec.TRANSPOSE_F32_ONLY:
        src = ec.finite_bf16(N * T * K, N + K + T).float()
        assert torch.isfinite(src).all()
        ref = ec.transpose_ref(src, N, K, T)
        assert ref.shape == (K, T, N) and ref[3 % K, 0, 2 % N] == src.view(N, T, K)[2 % N, T - 1, 3 % K]
        assert torch.equal(ec.transpose_ref(src, N, K, T, 'taps_not_reversed'), ref) == (T == 1)
    assert any(n % 64 and k % 64 and n % 8 == 0 and k % 8 == 0 for n, k, _ in ec.TRANSPOSE_CASES)
    tab, nj, nb = ec.tw_table([(16, 32, 72, 136, 9), (48, 64, 8, 200, 1)], 64)
    assert (nj, nb) == (2, 9 * 2 * 3 + 4) and tab.numel() == 2 * 32
    tab, nj, nb = ec.sc_table([(16, 32, 2049, 0.5), (48, 64, 1, 2.0)])
    assert (nj, nb) == (2, 3) and tab.numel() == 2 * 32


# ---- guard zones -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [BF16, F32], ids=['bf16', 'f32'])
def test_guard_zones_see_stray_and_missing_writes(dtype):
    g = ec.Guarded((3, 8), dtype, 'cpu')
    assert g.guards_intact() and not g.all_written() and g.untouched() and torch.isnan(g.buf.float()).all()
    assert g.ptr() % 16 == 0
    g.t.copy_(torch.ones(3, 8))
    assert g.guards_intact() and g.all_written()
    g.t[1, 2] = float('nan')                  # an ordinary NaN is a written value
    g.check()
    g.buf[g.lo + g.n] = 0
    assert not g.guards_intact()
    h = ec.Guarded(16, dtype, 'cpu', fill=ec.int_values((16,), 1))
    assert h.untouched() and h.all_written()
    h.t[15] += 1
    assert not h.untouched() and h.guards_intact()
    h.buf[h.lo - 1] = 1
    with pytest.raises(AssertionError):
        h.check()
    assert ec.Guarded(8, dtype, 'cpu', shift=1).ptr() % 16 == ec.Guarded(8, dtype, 'cpu').t.element_size()
