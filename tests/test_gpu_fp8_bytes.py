"""The e4m3 conversions byte for byte (cvt4_fp8 of csrc/common.h behind sidlsg_cast_fp8, sidlsg_quantize_fp8_rows and the fp8w loader):
every bf16 bit pattern through the cast, the whole e4m3 number line with its midpoints through the row quantisation at every power-of-two
scale, guard bytes behind every destination, and NaN -- which must stay NaN everywhere (include/sidlsg_hip.h, "fp8-weight contractions")."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp8_cases as fc      # noqa: E402
import gemm_cases as gc     # noqa: E402

pytestmark = pytest.mark.gpu
BF16, F32, F64, F8 = torch.bfloat16, torch.float32, torch.float64, torch.float8_e4m3fn
GUARD_BYTES = 64


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from sid_lsg_amd._lib import lib
    lib.load()
    return torch.device('cuda:0')


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _byte_dst(n, dev):
    return torch.full((n + GUARD_BYTES,), fc.GUARD_BYTE, dtype=torch.uint8, device=dev)


def _first(mask):
    return int(mask.nonzero()[0])


@pytest.mark.parametrize('name', ['8', '8x257', 'patterns', 'two_passes'])
def test_cast_fp8_every_pattern(dev, name):
    from sid_lsg_amd._lib import lib
    src = fc.cast_inputs()[name]
    n = src.numel()
    want = fc.ref_bytes(src)
    nan = torch.isnan(src.float())
    assert nan.any() and fc.is_nan_byte(want[nan]).all()
    x = src.to(dev)
    dst = _byte_dst(n, dev)
    lib.sidlsg_cast_fp8(x.data_ptr(), dst.data_ptr(), n, _stream())
    torch.cuda.synchronize()
    got = dst.cpu()
    assert (got[n:] == fc.GUARD_BYTE).all(), f'bytes behind the destination overwritten, first at +{_first(got[n:] != fc.GUARD_BYTE)}'
    got = got[:n]
    lost = nan & ~fc.is_nan_byte(got)
    assert not lost.any(), (f'{int(lost.sum())} of {int(nan.sum())} NaN inputs did not stay NaN; first: pattern 0x{int(src.view(torch.int16)[_first(lost)]) & 0xFFFF:04x} '
                            f'-> byte 0x{int(got[_first(lost)]):02x} ({got[_first(lost)].view(F8).float().item()})')
    bad = ~nan & (got != want)
    assert not bad.any(), (f'{int(bad.sum())} of {n} bytes differ; first at {_first(bad)}: {src[_first(bad)].item()!r} -> 0x{int(got[_first(bad)]):02x}, '
                           f'expected 0x{int(want[_first(bad)]):02x}')


def _quantize(lib, src, dev):
    rows, cols = src.shape
    x = src.to(dev).contiguous()
    dst = _byte_dst(rows * cols, dev)
    sc_whole, sc = gc.poisoned_flat(torch.zeros(rows, dtype=F32), dev)
    lib.sidlsg_quantize_fp8_rows(x.data_ptr(), dst.data_ptr(), sc.data_ptr(), rows, cols, _stream())
    torch.cuda.synchronize()
    got = dst.cpu()
    msgs = [gc.flat_damage(sc_whole, rows)]
    if not (got[rows * cols:] == fc.GUARD_BYTE).all():
        msgs.append('bytes behind dst overwritten')
    return got[:rows * cols].view(rows, cols), sc.cpu(), [m for m in msgs if m]


@pytest.mark.parametrize('cols', fc.QUANT_COLS)
@pytest.mark.parametrize('rows', fc.QUANT_ROWS)
def test_quantize_rows_number_line(dev, rows, cols):
    """Every finite e4m3 value and every midpoint, times 2^k, k = -12 .. 2 over the launches: the scale is 2^k exactly, the bytes are the
    nearest-even ones; a zero row gives scale 1 and zero bytes."""
    from sid_lsg_amd._lib import lib
    errors = []
    for k0 in range(0, len(fc.QUANT_K), rows):
        zero_row = rows // 2 if rows > 1 and k0 == 0 else None
        src, ks = fc.quant_rows(rows, cols, k0, zero_row=zero_row)
        want, want_scale = fc.quant_reference(src, ks)
        got, scale, msgs = _quantize(lib, src, dev)
        errors += [f'k0={k0}: {m}' for m in msgs]
        if not torch.equal(scale.view(torch.int32), want_scale.view(torch.int32)):
            errors.append(f'k0={k0}: scales {scale.tolist()}, expected 2^{ks.tolist()}')
        bad = got != want
        if bad.any():
            r, col = (int(i) for i in bad.nonzero()[0])
            errors.append(f'k0={k0}: {int(bad.sum())} bytes differ; first at ({r}, {col}): {src[r, col].item()!r} / 2^{int(ks[r])} -> 0x{int(got[r, col]):02x}, '
                          f'expected 0x{int(want[r, col]):02x}')
    assert not errors, '\n'.join(errors[:12])


@pytest.mark.parametrize('rows,cols,nan_at', [(1, 8, (0, 5)), (5, 520, (3, 515)), (7, 1032, (6, 0))])
def test_quantize_rows_keeps_nan(dev, rows, cols, nan_at):
    """The header's contract: a NaN entry becomes a NaN byte; the scale of its row (taken over the non-NaN entries) and every other byte stay."""
    from sid_lsg_amd._lib import lib
    src, ks = fc.quant_rows(rows, cols, 4, nan_at=nan_at)
    want, want_scale = fc.quant_reference(src, ks)
    got, scale, msgs = _quantize(lib, src, dev)
    assert not msgs, msgs
    assert torch.equal(scale.view(torch.int32), want_scale.view(torch.int32)), (scale.tolist(), want_scale.tolist())
    assert fc.is_nan_byte(got[nan_at]), f'the NaN became byte 0x{int(got[nan_at]):02x} ({got[nan_at].view(F8).float().item()})'
    keep = torch.ones(rows, cols, dtype=torch.bool)
    keep[nan_at] = False
    assert torch.equal(got[keep], want[keep])


@pytest.mark.parametrize('cid', ['fp8w-200x136x80', 'fp8wconv-2x12x20x80-136'])
def test_fp8w_loader_keeps_nan(dev, cid):
    """One NaN activation: exactly the output rows whose contraction reads it are NaN (all their channels), every other row stays exact."""
    from sid_lsg_amd import ops
    from sid_lsg_amd._lib import lib
    c = next(x for x in gc.FP8W_CASES if x['id'] == cid)
    M, N, K = gc.mnk(c)
    o = gc.fwd_operands(c)
    a = o['a'].clone()
    a.view(-1, a.shape[-1])[37, 70] = float('nan')          # (a channel of the K tail: past the first 64-wide K-tile)
    acc = gc.contract(c, a, o['w']) * o['wscale'].double()
    nan_rows = torch.isnan(acc).any(1)
    assert torch.equal(torch.isnan(acc), nan_rows[:, None].expand(M, N)) and int(nan_rows.sum()) == (1 if c['ep'] == 'gemm' else 9)
    _, w = gc.poisoned_flat(o['w'], dev)
    _, wscale = gc.poisoned_flat(o['wscale'], dev)
    ad = gc.poisoned(a.reshape(-1, a.shape[-1]), 8, dev)
    whole, out = gc.guarded(M, N, 8, F32, dev)
    p = dict(a=ad.data_ptr(), w=w.data_ptr(), wscale=wscale.data_ptr(), w1=None, wscale1=None, c=out.data_ptr(), bias=None, bias1=None, res=None, rv=None, stream=_stream())
    name, args = gc.fwd_call(c, 'f32_plain', None, p)
    ops.ensure_workspace(dev)
    getattr(lib, name)(*args)
    torch.cuda.synchronize()
    assert gc.guard_damage(whole, M, N) == ''
    got = out.contiguous().cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(acc)), f'NaN rows {torch.isnan(got).any(1).nonzero().flatten().tolist()}, expected {nan_rows.nonzero().flatten().tolist()}'
    assert torch.equal(got[~nan_rows].view(torch.int32), gc.round_out(acc[~nan_rows], F32).view(torch.int32))
