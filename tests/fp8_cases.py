"""Shared by tests/test_fp8_cases_host.py, tests/test_gpu_fp8_bytes.py and the e4m3 norm tests (not a test module): the OCP e4m3 number line
-- every finite value, every midpoint between neighbours -- the inputs of the byte-for-byte conversion tests built from it, and the
"decidable byte" oracle for kernels whose fp32 input to the conversion is itself only accurate to a tolerance.

The reference conversion is torch's CPU cast `x.float().clamp(-448, 448).to(float8_e4m3fn)`: round to nearest, ties to even, gradual
underflow below 2^-6; tests/test_fp8_cases_host.py checks that claim against the number line built here from the format's definition."""
import torch

BF16, F32, F64, F8 = torch.bfloat16, torch.float32, torch.float64, torch.float8_e4m3fn
E4M3_MAX = 448.0
GUARD_BYTE = 0xA5                     # what the bytes after a destination hold before and after a call
GUARD_F32 = 0x7FA55AA5                # the same for fp32 outputs: a NaN bit pattern (as int32)


def e4m3_decode(byte):
    """The value of an e4m3 byte by the format's definition (1 sign, 4 exponent bits of bias 7, 3 mantissa bits, no infinity; S.1111.111 is NaN)."""
    s, e, m = byte >> 7, (byte >> 3) & 15, byte & 7
    if e == 15 and m == 7:
        return float('nan')
    v = m * 2.0 ** -9 if e == 0 else (8 + m) * 2.0 ** (e - 10)
    return -v if s else v


def finite_values():
    """The 127 non-negative finite e4m3 values in byte order (0 .. 448), fp64."""
    return torch.tensor([e4m3_decode(b) for b in range(0x7F)], dtype=F64)


def midpoints():
    """The 126 midpoints between neighbouring non-negative values; midpoint i lies between bytes i and i + 1 and ties to the EVEN one."""
    v = finite_values()
    return (v[:-1] + v[1:]) / 2


def is_nan_byte(b):
    return (b & 0x7F) == 0x7F


def ref_bytes(x):
    """The contract: clamp to +-448, round to nearest even -> uint8 (NaN inputs give the NaN byte torch chooses; compare them with is_nan_byte)."""
    return x.float().clamp(-E4M3_MAX, E4M3_MAX).to(F8).view(torch.uint8)


def all_bf16_patterns():
    """Every bf16 bit pattern once, in pattern order -> bf16 [65536]."""
    return torch.arange(65536, dtype=torch.int32).to(torch.int16).view(BF16)


# ---- sidlsg_cast_fp8 -------------------------------------------------------------------------------------------------------------------
CAST_GRID_ELEMS = 8 * 256 * 4096      # elements one pass of cast_fp8_kernel's grid-stride loop covers at its largest grid
SPECIALS = (17.0, 19.0, 2.0 ** -10, 3 * 2.0 ** -10, 464.0, -0.0, float('nan'), 1e4)      # ties both ways, the underflow tie, past the range


def cast_inputs():
    """-> {name: bf16 vector}: 8 elements (one thread), 8 * 257 (a second block of one thread), every pattern, and just over one full pass."""
    pats = all_bf16_patterns()
    sp = torch.tensor(SPECIALS, dtype=F32).to(BF16)
    big = torch.cat([pats.repeat(CAST_GRID_ELEMS // 65536), pats[32760:32760 + 16], sp])      # (the 16 patterns around +inf / the first NaNs)
    return {'8': sp, '8x257': torch.cat([pats[::32], sp]), 'patterns': pats, 'two_passes': big}


# ---- sidlsg_quantize_fp8_rows ----------------------------------------------------------------------------------------------------------
QUANT_ROWS, QUANT_COLS, QUANT_K = (1, 5, 7), (8, 504, 512, 520, 1032), tuple(range(-12, 3))


def number_line_pool():
    """+- every finite value and every midpoint (505 distinct numbers), fp64; each has at most 5 significant bits: a bf16 value at every 2^k."""
    p = torch.cat([finite_values(), midpoints()])
    return torch.cat([p, -p[p > 0]])


def quant_rows(rows, cols, k0, zero_row=None, nan_at=None):
    """-> (src bf16 [rows, cols], k [rows]): row r holds pool values * 2^k[r] (k cycling through QUANT_K from k0), walks the pool from its own
    offset, and has +-448 * 2^k at one column (the row maximum, so the scale must be 2^k exactly).  zero_row: that row is all zeros (scale 1,
    k = 0); nan_at = (r, col): one NaN, which must neither move the scale nor vanish."""
    pool = number_line_pool()
    n = pool.numel()
    ks = torch.tensor([QUANT_K[(k0 + r) % len(QUANT_K)] for r in range(rows)])
    src = torch.empty(rows, cols, dtype=F64)
    for r in range(rows):
        src[r] = pool[(torch.arange(cols) + (k0 * 7 + r * 61) * 8) % n]
        src[r, (r * 37 + k0) % cols] = E4M3_MAX * (-1) ** r
        src[r] *= 2.0 ** int(ks[r])
    if zero_row is not None:
        src[zero_row] = 0
        ks[zero_row] = 0
    if nan_at is not None and nan_at[0] != zero_row:
        assert src[nan_at].abs() != E4M3_MAX * 2.0 ** int(ks[nan_at[0]])
        src[nan_at] = float('nan')
    out = src.to(BF16)
    assert torch.equal(out.double().nan_to_num(7.0), src.nan_to_num(7.0)), 'not bf16 values'
    return out, ks


def quant_reference(src, ks):
    """-> (bytes uint8 [rows, cols], scale fp32 [rows]) for rows built by quant_rows: x / 2^k is exact, so the only rounding is the conversion's."""
    scale = torch.pow(2.0, ks.double())
    return ref_bytes((src.double() / scale[:, None]).float()), scale.float()


# ---- kernels that convert a COMPUTED fp32 value (the e4m3-output norms) ------------------------------------------------------------------
def neighbours(y64):
    """-> (lo, hi) uint8: the bytes of the two e4m3 values that enclose clamp(y) (lo == hi where y is a value itself); negative y: by magnitude."""
    v = finite_values()
    a = y64.double().abs().clamp(max=E4M3_MAX)
    hi = torch.searchsorted(v, a)                      # first value >= a
    lo = torch.where(v[hi] == a, hi, hi - 1)
    sign = torch.where(y64 < 0, 0x80, 0).to(torch.uint8)
    return lo.to(torch.uint8) | sign, hi.to(torch.uint8) | sign


def decidable(y64, d):
    """Per element: the reference lies further than d from every midpoint between neighbouring e4m3 values, so any input within d of it rounds
    to the same byte.  d broadcasts against y64.  (Past +-448 everything saturates to the same byte: no midpoint there.)"""
    m = midpoints()
    a = y64.double().abs()
    i = torch.searchsorted(m, a).clamp(max=m.numel() - 1)
    near = torch.minimum((a - m[i]).abs(), (a - m[(i - 1).clamp(min=0)]).abs())
    return near > d


def byte_oracle(got_u8, y64, d):
    """-> (message or '', undecidable share).  A decidable element must be the reference's round-to-nearest-even byte, an undecidable one one of
    the two neighbouring bytes (which differ from the nearest-even byte only when the reference is within d of their midpoint)."""
    want = ref_bytes(y64.double().clamp(-E4M3_MAX, E4M3_MAX).float())
    dec = decidable(y64, d)
    lo, hi = neighbours(y64)
    got_u8 = got_u8.cpu()
    # a reference within d of zero does not decide the sign of a zero byte: both zero bytes are the same number there
    zero = lambda b: (b & 0x7F) == 0  # noqa: E731
    unsigned = (y64.double().abs() <= d) & zero(got_u8)
    same = (got_u8 == want) | (unsigned & zero(want))
    near = same | (got_u8 == lo) | (got_u8 == hi) | (unsigned & (zero(lo) | zero(hi)))
    bad = torch.where(dec, ~same, ~near)
    share = 1.0 - dec.double().mean().item()
    if not bad.any():
        return '', share
    idx = tuple(int(i) for i in bad.nonzero()[0])
    return (f'{int(bad.sum())} of {bad.numel()} bytes wrong ({int((bad & dec).sum())} decidable); first at {idx}: got 0x{int(got_u8[idx]):02x}, '
            f'reference {y64[idx].item():.6g} -> 0x{int(want[idx]):02x} (neighbours 0x{int(lo[idx]):02x}, 0x{int(hi[idx]):02x})'), share
