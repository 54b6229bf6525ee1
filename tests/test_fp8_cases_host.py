"""tests/fp8_cases.py checked on the CPU: the e4m3 number line against torch's cast (the reference conversion of the GPU tests rounds to
nearest, ties to even, saturates after the clamp), the inputs of the cast and row-quantisation tests, and the decidable-byte oracle."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp8_cases as fc      # noqa: E402

BF16, F32, F64, F8 = torch.bfloat16, torch.float32, torch.float64, torch.float8_e4m3fn


def test_number_line_is_torchs_e4m3():
    every = torch.arange(256, dtype=torch.int32).to(torch.uint8)
    mine = torch.tensor([fc.e4m3_decode(int(b)) for b in every], dtype=F64)
    theirs = every.view(F8).float().double()
    assert torch.equal(mine.nan_to_num(1e9), theirs.nan_to_num(1e9))
    assert torch.equal(torch.isnan(mine), fc.is_nan_byte(every)) and int(torch.isnan(mine).sum()) == 2
    v = fc.finite_values()
    assert v.numel() == 127 and v[0] == 0 and v[-1] == 448 and (v[1:] > v[:-1]).all()


def test_reference_conversion_rounds_to_nearest_even_and_saturates():
    v, m = fc.finite_values(), fc.midpoints()
    i = torch.arange(126)
    even = torch.where(i % 2 == 0, i, i + 1).to(torch.uint8)                         # of bytes i and i + 1 the even one
    assert torch.equal(fc.ref_bytes(m), even) and torch.equal(fc.ref_bytes(-m), even | 0x80)
    assert torch.equal(fc.ref_bytes(v), torch.arange(127).to(torch.uint8))
    up, down = torch.nextafter(m.float(), torch.tensor(1e9)), torch.nextafter(m.float(), torch.tensor(-1e9))
    assert torch.equal(fc.ref_bytes(up), (i + 1).to(torch.uint8)) and torch.equal(fc.ref_bytes(down), i.to(torch.uint8))
    x = torch.tensor([17.0, 19.0, 2.0 ** -10, 3 * 2.0 ** -10, 464.0, 1e4, float('inf'), -3e38])
    assert fc.ref_bytes(x).view(F8).float().tolist() == [16.0, 20.0, 0.0, 2.0 ** -8, 448.0, 448.0, 448.0, -448.0]
    assert int(fc.ref_bytes(torch.tensor([-0.0]))) == 0x80
    assert fc.is_nan_byte(fc.ref_bytes(torch.tensor([float('nan')]))).all()


def test_cast_inputs():
    inp = fc.cast_inputs()
    assert [v.numel() for v in inp.values()] == [8, 8 * 257, 65536, fc.CAST_GRID_ELEMS + 24]
    assert all(v.numel() % 8 == 0 and v.dtype == BF16 for v in inp.values())
    pats = inp['patterns'].view(torch.int16)
    assert pats.unique().numel() == 65536
    nan = torch.isnan(inp['patterns'].float())
    assert int(nan.sum()) == 2 * 127          # exponent all ones, mantissa not zero, either sign
    for v in inp.values():                    # every input holds a NaN, a tie that goes down, one that goes up, and a value past the range
        f = v.float()
        assert torch.isnan(f).any() and (f == 17).any() and (f == 19).any() and (f.abs() > 448).any()


def test_quantize_rows_cover_the_number_line():
    pool = fc.number_line_pool()
    assert pool.numel() == 505 and pool.unique().numel() == 505
    seen = set()
    for k0 in range(0, 15, 7):
        src, ks = fc.quant_rows(7, 1032, k0)
        want, scale = fc.quant_reference(src, ks)
        assert torch.equal(src.double().abs().amax(1), 448 * scale.double()) and torch.equal(scale.double(), torch.pow(2.0, ks.double()))
        unscaled = src.double() / scale.double()[:, None]
        assert set(unscaled.flatten().tolist()) == set(pool.tolist())                 # every value and midpoint, either sign, in every row
        assert torch.equal(want.view(F8).float().double(), fc.ref_bytes(unscaled.float()).view(F8).float().double())
        seen |= set(ks.tolist())
    assert seen == set(fc.QUANT_K)
    src, ks = fc.quant_rows(5, 8, 3, zero_row=2, nan_at=(4, 1))
    want, scale = fc.quant_reference(src, ks)
    assert (src[2] == 0).all() and scale[2] == 1 and (want[2] == 0).all()
    assert torch.isnan(src.float()).sum() == 1 and fc.is_nan_byte(want[4, 1]) and int(fc.is_nan_byte(want).sum()) == 1


def test_byte_oracle():
    g = torch.Generator().manual_seed(1)
    y = torch.randn(4000, generator=g, dtype=F64) * torch.pow(2.0, torch.randint(-1, 5, (4000,), generator=g).double())
    d = 1e-4 * y.abs().max()          # (one d for all: small values are undecidable more often, as in a norm's block)
    good = fc.ref_bytes(y.float())
    msg, share = fc.byte_oracle(good, y, d)
    assert msg == '' and 0 < share < 0.5
    dec = fc.decidable(y, d)
    lo, hi = fc.neighbours(y)
    assert ((good == lo) | (good == hi)).all()
    # a decidable byte moved to its other neighbour is rejected, an undecidable one is not
    other = torch.where(good == lo, hi, lo)
    i = int((dec & (other != good)).nonzero()[0])
    bad = good.clone(); bad[i] = other[i]
    assert 'decidable' in fc.byte_oracle(bad, y, d)[0]
    j = int((~dec & (other != good)).nonzero()[0])
    ok = good.clone(); ok[j] = other[j]
    assert fc.byte_oracle(ok, y, d)[0] == ''
    worse = good.clone(); worse[j] = (int(hi[j]) + 1) if int(hi[j]) & 0x7F < 0x7E else int(lo[j]) - 1
    assert fc.byte_oracle(worse, y, d)[0] != ''
    # within d of a midpoint means undecidable, and every perturbation of a decidable reference by less than d keeps its byte
    assert not fc.decidable(fc.midpoints()[5:60], 1e-12).any() and fc.decidable(fc.finite_values()[9:], 1e-4).all()
    for s in (-1, 1):
        moved = fc.ref_bytes((y + s * 0.999 * d).float())
        assert torch.equal(moved[dec & (y.abs() > d)], good[dec & (y.abs() > d)])
