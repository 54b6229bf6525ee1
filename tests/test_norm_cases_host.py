"""The cases of the distinct-statistics norm tests (tests/norm_cases.py) are checked here on the CPU, for every case the GPU tests use:

  * the tests can see what they are for: a reference made wrong on purpose -- statistics of the next group, statistics of the next
    sample, both projection terms of the backward dropped -- misses the tolerance of the GPU test by more than 10x;
  * the reference alone stays within: the fp64 result rounded once to bf16 is below half of every bf16 tolerance, and torch's own
    fp32 CPU group_norm / layer_norm is below half of every fp32 tolerance, under the metric of the GPU tests.

(The next-sample mutation needs a second sample: it is not applied at B = 1, where a wrong sample index reads outside the tensor.)
`pytest -s` prints every figure.
"""
import pytest
import torch

import norm_cases as nc

BF16_CASES = sorted(set(nc.GN_CASES_BF16 + nc.GN_CASES_DET), key=nc.GN_CASES_BF16.index)


def _mutations(B, G):
    return (['next_group'] if G > 1 else []) + (['next_sample'] if B > 1 else []) + ['no_projection']


def _check_mutations(c, shape3, G, eps, silu, tol, rel):
    """c: a case dict with 3-d views; rel(got, ref) the per-block metric."""
    x, dy = c['x'].view(shape3), c['dy'].view(shape3)
    ref = {k: v.reshape(shape3) if v.dim() != 1 else v for k, v in c['ref'].items()}
    if c.get('dk') is not None:
        ref = dict(ref, dx=ref['dx'] - c['dk'].double().view(shape3))      # (the residual-branch gradient is not part of the formula)
    ok = nc.norm_by_formula(x, dy, c['gam'], c['bet'], G, eps, silu)
    for k in ('y', 'dx'):
        assert rel(ok[k], ref[k]) < 1e-9, f'the written-out formula differs from autograd in {k}'
    for k in ('dgamma', 'dbeta'):
        assert nc.global_rel_err(ok[k], ref[k]) < 1e-9, f'the written-out formula differs from autograd in {k}'
    for m in _mutations(shape3[0], G):
        bad = nc.norm_by_formula(x, dy, c['gam'], c['bet'], G, eps, silu, mutation=m)
        errs = {k: rel(bad[k], ref[k]) for k in (('dx',) if m == 'no_projection' else ('y', 'dx'))}
        print(f'  mutation {m}: ' + ', '.join(f'{k} {v:.3g} ({v / tol[k]:.0f}x tol)' for k, v in errs.items()))
        for k, v in errs.items():
            assert v > 10 * tol[k], f'{m}: {k} error {v:.3g} is not above 10 x {tol[k]}: the GPU test could miss this bug'


def _check_bf16_rounding(ref, rel):
    for k in ('y', 'dx'):
        e = rel(ref[k].to(nc.BF16), ref[k])
        print(f'  fp64 {k} rounded to bf16: {e:.3g}')
        assert e < 0.5 * nc.TOL_BF16[k], f'{k}: the reference rounded to bf16 is at {e:.3g}, not below half of {nc.TOL_BF16[k]}'


@pytest.mark.parametrize('case', BF16_CASES, ids=nc.gn_id)
def test_groupnorm_bf16_cases(case):
    B, HW, C, G, silu, eps, fork = case
    c = nc.gn_case(case, nc.OFFSETS_BF16, nc.BF16)
    rel = lambda got, ref: nc.group_rel_err(got, ref, G)  # noqa: E731
    _check_mutations(c, (B, HW, C), G, eps, silu, nc.TOL_BF16, rel)
    _check_bf16_rounding(c['ref'], rel)


@pytest.mark.parametrize('case', nc.LN_CASES_BF16, ids=lambda c: f'{c[0]}-{c[1]}')
def test_layernorm_bf16_cases(case):
    rows, C = case
    c = nc.ln_case(case, nc.OFFSETS_BF16, nc.BF16)
    rel = lambda got, ref: nc.row_rel_err(got.reshape(rows, C), ref.reshape(rows, C))  # noqa: E731
    _check_mutations(c, (rows, 1, C), 1, 1e-5, 0, nc.TOL_BF16, rel)
    _check_bf16_rounding(c['ref'], rel)


def _check_torch_f32(got, ref, rel, tol, what):
    errs = dict(y=rel(got['y'], ref['y']), dx=rel(got['dx'], ref['dx']),
                dgamma=nc.global_rel_err(got['dgamma'], ref['dgamma']), dbeta=nc.global_rel_err(got['dbeta'], ref['dbeta']))
    print(f'NORM_ACCURACY torch_cpu_fp32 {what} ' + ' '.join(f'{k}={v:.3g}' for k, v in errs.items()))
    for k, v in errs.items():
        assert v < 0.5 * tol[k], f'{k}: torch fp32 is at {v:.3g}, not below half of the tolerance {tol[k]:.3g}'


@pytest.mark.parametrize('name,offsets,factor', nc.OFFSET_SETS_F32, ids=[s[0] for s in nc.OFFSET_SETS_F32])
@pytest.mark.parametrize('case', nc.GN_CASES_F32, ids=nc.gn_id)
def test_groupnorm_f32_cases(case, name, offsets, factor):
    B, HW, C, G, silu, eps, fork = case
    c = nc.gn_case(case, offsets, nc.F32)
    tol = {k: v * factor for k, v in nc.TOL_F32.items()}
    rel = lambda got, ref: nc.group_rel_err(got, ref, G)  # noqa: E731
    _check_mutations(c, (B, HW, C), G, eps, silu, tol, rel)
    t32 = nc.gn_reference(c['x'], c['dy'], c['gam'], c['bet'], G, eps, silu, dtype=nc.F32)
    _check_torch_f32(t32, c['ref'], rel, tol, f'gn {nc.gn_id(case)} {name}')


@pytest.mark.parametrize('name,offsets,factor', nc.OFFSET_SETS_F32, ids=[s[0] for s in nc.OFFSET_SETS_F32])
@pytest.mark.parametrize('case', nc.LN_CASES_F32, ids=lambda c: f'{c[0]}-{c[1]}')
def test_layernorm_f32_cases(case, name, offsets, factor):
    rows, C = case
    c = nc.ln_case(case, offsets, nc.F32)
    tol = {k: v * factor for k, v in nc.TOL_F32.items()}
    rel = lambda got, ref: nc.row_rel_err(got.reshape(rows, C), ref.reshape(rows, C))  # noqa: E731
    _check_mutations(c, (rows, 1, C), 1, 1e-5, 0, tol, rel)
    t32 = nc.ln_reference(c['x'], c['dy'], c['gam'], c['bet'], 1e-5, dtype=nc.F32)
    _check_torch_f32(t32, c['ref'], rel, tol, f'ln {rows}-{C} {name}')


F8_CASES = nc.f8_cases()


def test_e4m3_case_lists_are_complete():
    """The lists are filtered out of GN_CASES_BF16 and of the ids: an edit there must not drop a case silently."""
    ids = [c[0] for c in F8_CASES]
    assert len(nc.GN_CASES_F8) == 6 and len(nc.LN_CASES_F8) == 3 and len(F8_CASES) == 11 and len(set(ids)) == 11
    assert len(nc.F8_NAN_IDS) == 4 and set(nc.F8_NAN_IDS) <= set(ids)
    assert sum(c[3] != 1.0 for c in F8_CASES) == 2
    assert 1.0e-4 < nc.F8_STATS_TOL < 1.1e-4


@pytest.mark.parametrize('cid,kind,case,gain', F8_CASES, ids=[c[0] for c in F8_CASES])
def test_e4m3_forward_cases(cid, kind, case, gain):
    """The byte oracle of the e4m3-output forwards on the reference alone: the undecidable share stays under the cap, the reference's own bytes
    pass, bytes of a forward that used the next group's / next sample's statistics do not, and the saturating cases saturate."""
    import fp8_cases as fc
    c = nc.f8_case(kind, case, gain)
    x, y, G = c['x'], c['y'], c['G']
    B = x.shape[0]
    zero = torch.zeros_like(x)
    auto = nc.gn_reference(x, zero, c['gam'], c['bet'], G, c['eps'], c['silu'])['y']
    assert nc.group_rel_err(y, auto, G) < 1e-12, 'the written-out formula differs from F.group_norm'
    d = nc.block_d(y, G)
    msg, share = fc.byte_oracle(fc.ref_bytes(y.float()), y, d)
    sat = min(int((y >= 448).sum()), int((y <= -448).sum()))
    print(f'  {cid}: undecidable {100 * share:.2f} %, saturated outputs per sign >= {sat}')
    assert msg == '' and share <= nc.F8_UNDECIDABLE_CAP, (msg, share)
    if gain != 1.0:
        want = fc.ref_bytes(y.float())
        assert (int((want == 0x7E).sum()), int((want == 0xFE).sum())) == nc.F8_SAT_COUNTS[kind] and sat >= 5
        lo, hi = nc.f8_sat_bounds(y, d)
        assert all(0 < a <= b for a, b in zip(lo, hi)) and all(a <= n <= b for a, n, b in zip(lo, nc.F8_SAT_COUNTS[kind], hi)), (lo, hi)
    else:
        assert y.abs().max() < 448
    for m in (['next_group'] if G > 1 else []) + (['next_sample'] if B > 1 else []):
        bad = nc.norm_by_formula(x, zero, c['gam'], c['bet'], G, c['eps'], c['silu'], mutation=m)['y']
        msg, _ = fc.byte_oracle(fc.ref_bytes(bad.float()), y, d)
        assert 'decidable' in msg and int(msg.split(' of ')[0]) > 0.2 * y.numel(), f'{m}: {msg!r}'
    # (the third wrong reference of this file, no_projection, only changes dx: the forward it describes is the right one)
    assert torch.equal(nc.norm_by_formula(x, zero, c['gam'], c['bet'], G, c['eps'], c['silu'], mutation='no_projection')['y'], y)
    # the bf16 forward's bar on the statistics notices the same two mutations
    mean, rstd = c['mean'], c['rstd']
    for shift, dims in ((1, G > 1), (0, B > 1)):
        if dims:
            e = max(((mean.roll(-1, shift) - mean).abs() * rstd).max().item(), (rstd.roll(-1, shift) / rstd - 1).abs().max().item())
            assert e > 10 * nc.F8_STATS_TOL


def test_every_offset_and_scale_is_used():
    """The generator's promise: each case sees every offset of its list and more than one scale."""
    for case in nc.GN_CASES_BF16:
        B, HW, C, G = case[:4]
        x, _ = nc.structured_gn(B, HW, C, G, nc.case_seed(case), nc.OFFSETS_BF16, nc.F64)
        xg = x.view(B, HW, G, C // G)
        mean, std = xg.mean(dim=(1, 3)), xg.std(dim=(1, 3))
        got = set((mean / std).round().int().flatten().tolist())
        # (|offset| = 30 is only resolved to ~1 by the sample statistics of the smallest groups)
        assert any(o >= 28 for o in got) and any(o <= -28 for o in got) and 0 in got and 3 in got and -3 in got, (case, sorted(got))
        assert len(set(torch.log2(std).round().int().flatten().tolist())) >= 3, case
