"""The e4m3-output norms (sidlsg_groupnorm_fwd_fp8 / sidlsg_layernorm_fwd_fp8: the F8 instantiations of csrc/norm.hip) against the fp64 reference
of the distinct-statistics inputs of tests/norm_cases.py, byte for byte: every decidable output is the reference's round-to-nearest-even byte, an
undecidable one (reference within the fp32 bar of a midpoint) one of the two neighbours; outputs past +-448 saturate; a NaN input makes the
outputs of its (sample, group) / row NaN bytes and leaves every other block alone."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp8_cases as fc      # noqa: E402
import norm_cases as nc     # noqa: E402

pytestmark = pytest.mark.gpu
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
GUARD_BYTES = 64
CASES = nc.f8_cases()


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from sid_lsg_amd._lib import lib
    lib.load()
    return torch.device('cuda:0')


def _forward(dev, kind, c, x):
    """-> (y8 uint8 [B, HW, C] on the CPU, stats fp32 [B, G, 2] on the CPU, guard message)."""
    from sid_lsg_amd._lib import lib
    B, HW, C = x.shape
    G = c['G']
    st = torch.cuda.current_stream().cuda_stream
    xd, gam, bet = x.to(dev).contiguous(), c['gam'].to(dev), c['bet'].to(dev)
    y = torch.full((x.numel() + GUARD_BYTES,), fc.GUARD_BYTE, dtype=torch.uint8, device=dev)
    stats = torch.full((B * G * 2 + 8,), fc.GUARD_F32, dtype=torch.int32, device=dev).view(F32)
    if kind == 'gn':
        n = lib.sidlsg_groupnorm_ws_floats.raw(B, HW, C, G)
        assert n >= 0
        ws = torch.full((max(n, 1),), float('nan'), device=dev)
        lib.sidlsg_groupnorm_fwd_fp8(xd.data_ptr(), gam.data_ptr(), bet.data_ptr(), y.data_ptr(), stats.data_ptr(), ws.data_ptr(), B, HW, C, G, float(c['eps']),
                                     int(c['silu']), st)
    else:
        lib.sidlsg_layernorm_fwd_fp8(xd.data_ptr(), gam.data_ptr(), bet.data_ptr(), y.data_ptr(), stats.data_ptr(), B, C, float(c['eps']), st)
    torch.cuda.synchronize()
    y, stats = y.cpu(), stats.cpu()
    damage = '' if (y[x.numel():] == fc.GUARD_BYTE).all() and (stats[B * G * 2:].view(torch.int32) == fc.GUARD_F32).all() else 'bytes behind y8 or stats overwritten'
    return y[:x.numel()].view(B, HW, C), stats[:B * G * 2].view(B, G, 2), damage


@pytest.mark.parametrize('cid,kind,case,gain', CASES, ids=[c[0] for c in CASES])
def test_e4m3_forward_bytes(dev, cid, kind, case, gain):
    c = nc.f8_case(kind, case, gain)
    y8, stats, damage = _forward(dev, kind, c, c['x'])
    assert not damage, damage
    # statistics: fp32 (mean, rstd) per block against fp64, at what fp32 arithmetic on these offsets can cost (norm_cases.F8_STATS_TOL)
    e_mean = ((stats[..., 0].double() - c['mean']).abs() * c['rstd']).max().item()
    e_rstd = (stats[..., 1].double() / c['rstd'] - 1).abs().max().item()
    msg, share = fc.byte_oracle(y8, c['y'], nc.block_d(c['y'], c['G']))
    print(f'NORM_E4M3 {cid} mean err / sigma {e_mean:.3g} rstd rel err {e_rstd:.3g} undecidable {100 * share:.2f} %')
    assert e_mean <= nc.F8_STATS_TOL and e_rstd <= nc.F8_STATS_TOL, (e_mean, e_rstd)
    assert share <= nc.F8_UNDECIDABLE_CAP
    assert msg == '', msg
    if gain != 1.0:          # the share of saturated outputs: the number of +-448 bytes against the reference's own count (norm_cases.f8_sat_bounds)
        y = c['y']
        lo, hi = nc.f8_sat_bounds(y, nc.block_d(y, c['G']))
        got = (int((y8 == 0x7E).sum()), int((y8 == 0xFE).sum()))
        print(f'NORM_E4M3 {cid} +-448 bytes {got}, reference {lo} .. {hi}')
        assert all(a <= n <= b for a, n, b in zip(lo, got, hi)), (got, lo, hi)


NAN_CASES = [c for c in CASES if c[0] in nc.F8_NAN_IDS]


@pytest.mark.parametrize('cid,kind,case,gain', NAN_CASES, ids=[c[0] for c in NAN_CASES])
def test_e4m3_forward_keeps_nan(dev, cid, kind, case, gain):
    c = nc.f8_case(kind, case, gain)
    x = c['x'].clone()
    B, HW, C = x.shape
    G = c['G']
    b, p, ch = (B - 1 if kind == 'gn' else B // 3), HW // 3, C - 3          # the last group of the last sample; a row in the middle
    x[b, p, ch] = float('nan')
    g = ch // (C // G)
    y8, stats, damage = _forward(dev, kind, c, x)
    assert not damage, damage
    blocks = y8.view(B, HW, G, C // G)
    hit = torch.zeros(B, 1, G, 1, dtype=torch.bool)
    hit[b, 0, g, 0] = True
    hit = hit.expand(B, HW, G, C // G)
    nan = fc.is_nan_byte(blocks)
    assert nan[hit].all(), f'{int((~nan[hit]).sum())} of {int(hit.sum())} outputs of the block with the NaN input are numbers; first bytes {blocks[hit][:8].tolist()}'
    assert not nan[~hit].any(), 'a NaN byte outside the block of the NaN input'
    keep = (~hit).reshape(B, HW, C)
    y = c['y']
    msg, _ = fc.byte_oracle(y8[keep], y[keep], nc.block_d(y, G)[keep])
    assert msg == '', msg
