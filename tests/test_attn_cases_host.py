"""The cases of the attention tests (tests/attn_cases.py) are checked here on the CPU, for every case the GPU tests use:

  * the inputs probe something: the needle key's softmax share lies in [0.005, 0.97] for every query of every (batch, head) pair
    (all of them where two keys or more exist);
  * the bounds can be met: the CPU emulation of the kernels' rounding (attn_emulated) passes close_slices against the fp64 reference
    at the bounds of the GPU tests, and the whole-tensor close(..., 2e-2) of tests/test_gpu_ops.py as well; GRAD_TOL is what the
    module says it is, twice the emulation's largest per-slice error with a floor of 2e-2 and a ceiling of 5e-2;
  * the GPU tests can fail: a reference made wrong on purpose -- the needle key dropped, counted twice, the last key masked, the
    value rows of the needle and its neighbour swapped -- misses the bound by more than 10x in the output and in at least one
    gradient; with the biased input one all-zero key row appended misses the forward and the LSE bound by more than 10x.

`pytest -s` prints every figure.
"""
import pytest
import torch

import attn_cases as ac

_emu_errs = {}


def _emulation_errors(c):
    if c not in _emu_errs:
        x, ref = ac.case_data(c)
        emu = ac.attn_emulated(x['q'], x['k'], x['v'], x['do'], c.H, c.ps)
        e = {n: ac.slice_rel_err(emu[n], ref[n], c.H) for n in ('o', 'dq', 'dk', 'dv')}
        e['lse'] = ac.lse_err_bits(emu['lse2'], ref['lse2'])
        for n in ('dq', 'dk', 'dv'):          # the second assertion of the GPU tests: the whole tensor at 2e-2
            scale = ref[n].abs().max().item()
            e['whole_' + n] = (emu[n].double() - ref[n]).abs().max().item() / scale if scale > 1e-12 else 0.0
        _emu_errs[c] = e
    return _emu_errs[c]


def _check_share(share, what):
    lo, hi = share.min().item(), share.max().item()
    print(f'  {what}: needle share min {lo:.4f} median {share.median().item():.3f} max {hi:.4f}')
    assert ac.SHARE_RANGE[0] <= lo and hi <= ac.SHARE_RANGE[1], f'{what}: needle share {lo:.4g} .. {hi:.4g} is outside {ac.SHARE_RANGE}'


@pytest.mark.parametrize('c', ac.GRAD_CASES, ids=ac.case_id)
def test_needle_case(c):
    x, ref = ac.case_data(c)
    if c.Nk >= 2:
        _check_share(ref['share'], ac.case_id(c))
    e = _emulation_errors(c)
    print('  emulation: ' + ' '.join(f'{n}={v:.4f}' for n, v in e.items()))
    assert e['o'] <= ac.FWD_TOL and e['lse'] <= ac.LSE_TOL_BITS
    for n in ('dq', 'dk', 'dv'):
        assert e[n] <= ac.GRAD_TOL[n], f'{n}: the emulation is at {e[n]:.3g} per slice, above {ac.GRAD_TOL[n]}'
        assert e['whole_' + n] <= ac.WHOLE_GRAD_TOL, n
    if c.Nk < 2:
        return
    for m in ac.MUTATIONS:
        bad = ac.attn_ref64(x['q_ref'], x['k'], x['v'], x['do'], c.H, pos=x['pos'], mutation=m)
        eo = ac.slice_rel_err(bad['o'], ref['o'], c.H) / ac.FWD_TOL
        eg = {n: ac.slice_rel_err(bad[n], ref[n], c.H) / ac.GRAD_TOL[n] for n in ('dq', 'dk', 'dv')}
        print(f'  mutation {m}: o {eo:.0f}x tol, ' + ', '.join(f'{n} {v:.0f}x' for n, v in eg.items()))
        assert eo > 10, f'{m}: the output error is only {eo:.1f}x its bound: the GPU test could miss this bug'
        assert max(eg.values()) > 10, f'{m}: no gradient is further than 10x its bound ({eg})'


@pytest.mark.parametrize('c', ac.BIASED_CASES, ids=ac.case_id)
def test_biased_case(c):
    x = ac.make_inputs(c, 'biased')
    ref = ac.attn_ref64(x['q_ref'], x['k'], x['v'], x['do'], c.H, pos=x['pos'], grads=False)
    if c.Nk >= 2:
        _check_share(ref['share'], ac.case_id(c))
    # every real score lies 12 nats lower than a zero row's
    top = ref['lse2'].max().item() / ac.LOG2E
    assert top < -ac.BIAS_NATS + 9.0, f'log-sum-exp {top:.2f} nats: the bias is gone'
    emu = ac.attn_emulated(x['q'], x['k'], x['v'], x['do'], c.H, c.ps, grads=False)
    eo, el = ac.slice_rel_err(emu['o'], ref['o'], c.H), ac.lse_err_bits(emu['lse2'], ref['lse2'])
    print(f'  emulation: o={eo:.4f} lse={el:.4f} bits')
    assert eo <= ac.FWD_TOL and el <= ac.LSE_TOL_BITS
    bad = ac.attn_ref64(x['q_ref'], x['k'], x['v'], x['do'], c.H, mutation='zero_row', grads=False)
    eo, el = ac.slice_rel_err(bad['o'], ref['o'], c.H), ac.lse_err_bits(bad['lse2'], ref['lse2'])
    print(f'  one phantom key: o {eo / ac.FWD_TOL:.0f}x tol, lse {el / ac.LSE_TOL_BITS:.0f}x tol')
    assert eo > 10 * ac.FWD_TOL and el > 10 * ac.LSE_TOL_BITS


@pytest.mark.parametrize('c', ac.F32_CASES, ids=ac.case_id)
def test_f32_case(c):
    x, ref = ac.case_data(c, dtype=ac.F32)
    _check_share(ref['share'], ac.case_id(c))
    for m in ac.MUTATIONS:
        bad = ac.attn_ref64(x['q_ref'], x['k'], x['v'], x['do'], c.H, pos=x['pos'], mutation=m)
        for n in ('o', 'dv'):
            assert ac.slice_rel_err(bad[n], ref[n], c.H) > 10 * ac.FWD_TOL, (m, n)      # (the bf16 bound: 600x the fp32 one)


@pytest.mark.parametrize('c', ac.CAUSAL_CASES, ids=ac.case_id)
def test_causal_case(c):
    """Queries in front of the needle do not see it (share 0); from the needle on every query does, and the last one sees other
    keys as well.  Dropping the needle, and a mask that is off by one key (every query also sees its successor), miss the bound."""
    x, ref = ac.case_data(c, causal=True, grads=False)
    N = c.Nq
    qi = torch.arange(N).view(1, 1, N)
    after = qi >= x['pos'].unsqueeze(-1)
    assert (ref['share'][~after] == 0).all()
    assert ref['share'][after].min().item() >= ac.SHARE_RANGE[0] and ref['share'][..., -1].max().item() <= ac.SHARE_RANGE[1]
    assert sorted(set(x['pos'].flatten().tolist())) == sorted({0, 15, 16, N - 1})
    bad = ac.attn_ref64(x['q_ref'], x['k'], x['v'], x['do'], c.H, pos=x['pos'], causal=True, mutation='drop', grads=False)
    rows = after.transpose(1, 2).reshape(c.B, N, c.H, 1).expand(c.B, N, c.H, c.D).reshape(c.B, N, c.H * c.D)
    # (a query that sees the needle alone has no key left: compare where the mutant is finite)
    ok = torch.isfinite(bad['o'])
    assert ac.slice_rel_err(torch.where(ok, bad['o'], ref['o']), ref['o'], c.H) > 10 * ac.FWD_TOL
    assert torch.equal(bad['o'][~rows & ok], ref['o'][~rows & ok])
    # off by one: the reference of N + 1 keys' mask shifted -- computed as the causal attention with the keys rolled by one
    k1, v1 = x['k'].roll(-1, 1), x['v'].roll(-1, 1)
    off = ac.attn_ref64(x['q_ref'], k1, v1, x['do'], c.H, causal=True, grads=False)
    assert ac.slice_rel_err(off['o'], ref['o'], c.H) > 10 * ac.FWD_TOL


def test_positions_cover_the_edges():
    """Over the launches of one DP (both widths, plain and `_ps`, N = 200 and 128) the needle sits on every listed key; every launch
    has the last key; the Nk >= 1024 launches have a key in the second 64 of a 128-key block."""
    for dp in ac.ADMITTED_DP:
        for N in (200, 128):
            seen = set()
            for c in ac.SWEEP_CASES:
                if (c.D + 15) // 16 * 16 == dp and c.Nk == N:
                    p = ac.needle_positions(c)
                    assert p[0] == N - 1 and len(p) == c.B * c.H
                    seen.update(p)
            assert {0, 15, 16, 31, 32, 63, 64, N - 1, N - 2, N // 2} <= seen, (dp, N, sorted(seen))
    for c in ac.SWEEP_CASES + ac.EDGE_CASES + ac.LONG_CASES + ac.FUSED_CASES:
        assert ac.needle_positions(c)[0] == c.Nk - 1
    for c in ac.LONG_CASES + ac.FUSED_CASES:
        if c.Nk >= 1024:
            assert ac.needle_positions(c)[1] % 128 >= 64
    # every edge width sees every listed key over its edge lengths
    for D in ac.EDGE_D:
        seen = set()
        for c in ac.SWEEP_CASES + ac.EDGE_CASES:
            if c.D == D:
                seen.update(ac.needle_positions(c))
        assert {0, 15, 16, 31, 32, 63, 64} <= seen, (D, sorted(seen))


def test_case_tables():
    assert len(ac.WIDTHS) == 16 and not set(ac.WIDTHS) & set(ac.REFUSED_WIDTHS)
    assert {c.D for c in ac.SWEEP_CASES} == set(ac.WIDTHS)
    for dp in ac.ADMITTED_DP:       # both forwards of every DP: with the ones column (D = DP - 8) and without (D = DP)
        assert {ac.is_ones(c.D) for c in ac.SWEEP_CASES if (c.D + 15) // 16 * 16 == dp} == {True, False}
    assert max(max(c.Nq, c.Nk) for c in ac.GRAD_CASES + ac.BIASED_CASES + ac.F32_CASES + ac.CAUSAL_CASES) <= 1536


def test_gradient_bounds_are_the_measured_ones():
    worst = {n: max(_emulation_errors(c)[n] for c in ac.GRAD_CASES) for n in ('dq', 'dk', 'dv')}
    print('largest per-slice error of the emulation: ' + ' '.join(f'{n}={v:.5f}' for n, v in worst.items()))
    for n, v in worst.items():
        want = max(ac.GRAD_TOL_FLOOR, 2 * v)
        assert want <= ac.GRAD_TOL[n] <= min(1.05 * want, ac.GRAD_TOL_CEILING), f'{n}: bound {ac.GRAD_TOL[n]}, measured {v:.5f} -> {want:.4f}'


def test_header_ops_and_case_tables_agree_on_the_admitted_widths():
    import os
    from sid_lsg_amd import ops
    assert ops.ATTN_HEAD_WIDTHS == ac.ADMITTED_DP
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'sidlsg_hip.h')).read()
    assert 'round-up to a multiple of 16 is one of ' + ', '.join(map(str, ac.ADMITTED_DP[:-1])) + f' or {ac.ADMITTED_DP[-1]}' in header
    for D in ac.WIDTHS + ac.F32_WIDTHS:
        ops._attn_head_width(D, ac.F32 if D % 8 else ac.BF16)
    for D in ac.REFUSED_WIDTHS:
        with pytest.raises(RuntimeError, match='not admitted'):
            ops._attn_head_width(D, ac.BF16)
