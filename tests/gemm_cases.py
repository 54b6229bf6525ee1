"""Shared by tests/test_gemm_cases_host.py and tests/test_gpu_gemm_exact.py (not a test module): EXACT cases for the bf16 GEMM / conv3x3 /
weight-gradient family of csrc/gemm.hip, csrc/wgrad.hip and csrc/gemm_p8.h and for the e4m3 kernels of csrc/gemm_fp8.hip, the dispatch record
every case must produce, and guarded buffers.

Exact operands.  Activations and dY are integers in [-3, 3], weights integers in [-2, 2], all stored as bf16; bias, row vector and the
previous contents of an accumulated output are integer-valued fp32, the residual is integer-valued bf16, alpha is 1, 0.5 or 2.  Every
product and every partial sum, in ANY order, is then an integer (or a half) far below 2^24, which fp32 holds exactly: whatever tile
shape, K-split slab order or fp32-atomic order a correct kernel uses, it must produce THE result -- an fp32 output bit-equal to the
fp64 reference, a bf16 output bit-equal to the reference rounded once to nearest-even.  No tolerance is measured or chosen anywhere;
the one exception is SiLU (not exact), which keeps the 1.2e-2 bar of tests/test_gpu_ops.py.  Bias and residual reach about 1000, so
that a bf16 output needs rounding (and meets ties) at every K; tests/test_gemm_cases_host.py asserts that per case.

Which kernel ran.  Every row of the tables names the dispatch record (include/sidlsg_hip.h sidlsg_debug_last_launch) it must produce.
A row that reaches another kernel FAILS (it never skips): a retuned threshold cannot move coverage silently.  The host test checks the
records without a GPU (the record is written before the launch), the GPU test checks them again next to the results.

Memory around the operands.  Outputs live in a buffer of M + GUARD rows of ldc = N + pad elements filled with a sentinel bit pattern (a
NaN); inputs have row strides wider than their logical width, the padding columns and GUARD rows after the last row hold NaN; the
split-K workspace is NaN-filled.  After a call every element outside [0, M) x [0, N) must still be the sentinel and no NaN may have
reached the output.

e4m3 rows (FP8W_CASES, MX8_CASES).  The entry points take the e4m3 BYTES and the per-channel scale vector, so the operands stay exact:
weights are e4m3 bytes of integers in [-2, 2], activations e4m3 bytes of integers in [-3, 3] (mx8) or bf16 integers the loader converts
(fp8w), wscale[n] cycles through a short list of powers of two and small integers whose period divides no tile, fragment or wave width.
Every product, partial sum and wscale[n] * acc is then exact in fp32 in any order and the reference is alpha * wscale[n] * acc followed by
the same epilogue chain.  Padding bytes and guard rows of an e4m3 operand are 0x7F, the e4m3 NaN: a chunk read past K or Cin that reaches
the MFMA shows up as a NaN in the output."""
import ctypes
import functools
import os
import re

import torch
import torch.nn.functional as F

BF16, F32, F64, F8 = torch.bfloat16, torch.float32, torch.float64, torch.float8_e4m3fn
OUT_F32, SILU, ACCUM = 1, 2, 4
GUARD = 3                          # rows after the last logical row of every guarded buffer
SENTINEL = {BF16: 0x7FA5, F32: 0x7FA55AA5, F8: 0x7F}          # NaN bit patterns (bf16 as int16, fp32 as int32, e4m3 as uint8)
INT_OF = {BF16: torch.int16, F32: torch.int32, F8: torch.uint8}
SILU_TOL = 1.2e-2                  # max|err| / max|ref|, the bf16 bar of tests/test_gpu_ops.py
WORKSPACE_BYTES = 512 << 20        # what ops.ensure_workspace registers; the dispatch rules depend on it

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'sidlsg_hip.h')


# ---- the dispatch record -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def header_enums():
    """-> {name: value} for every `SIDLSG_X = n` enumerator of the header (comments stripped)."""
    src = re.sub(r'/\*.*?\*/', ' ', open(HEADER).read(), flags=re.S)
    return {m.group(1): int(m.group(2)) for m in re.finditer(r'\b(SIDLSG_[A-Z0-9_]+)\s*=\s*(\d+)', src)}


def kernel_ids():
    """-> {id: short name} of enum sidlsg_kernel_id, e.g. {2: 'GEMM_V3'}."""
    return {v: k[len('SIDLSG_K_'):] for k, v in header_enums().items() if k.startswith('SIDLSG_K_')}


REC_FIELDS = ('kernel', 'bm', 'bn', 'mode', 'pad', 'p8', 'splits', 'partial', 'finish', 'seq')
PART = {0: 'one', 1: 'slabs', 2: 'atomics'}
FIN_GEMM, FIN_REDUCE, FIN_COLSUM = 1, 2, 4


def last_launch(lib):
    """The calling thread's dispatch record as a dict (kernel and partial by name)."""
    e = header_enums()
    n = e['SIDLSG_REC_INTS']
    assert [e['SIDLSG_REC_' + f.upper()] for f in REC_FIELDS] == list(range(n))
    buf = (ctypes.c_int * n)()
    got = lib.sidlsg_debug_last_launch.raw(ctypes.addressof(buf), n)
    assert got == n, f'sidlsg_debug_last_launch returned {got}'
    r = dict(zip(REC_FIELDS, list(buf)))
    r['kernel'] = kernel_ids()[r['kernel']]
    r['partial'] = PART[r['partial']]
    return r


def rec(kernel, bm, bn, mode, splits=1, partial=None, finish=None, pad=-1, p8=-1):
    """An expected record.  GEMM family: `splits` > 1 means slabs + gemm_finish_kernel.  Weight gradients say `partial` themselves."""
    if partial is None:
        partial = 'slabs' if splits > 1 else 'one'
    if finish is None:
        finish = 0 if partial != 'slabs' else (FIN_REDUCE if kernel.startswith('WGRAD') else FIN_GEMM)
    return dict(kernel=kernel, bm=bm, bn=bn, mode=mode, pad=pad, p8=p8, splits=splits, partial=partial, finish=finish)


def record_mismatch(case_id, got, want):
    """'' when the record is the expected one, else the message of the failing assertion: the shape and both kernels."""
    diff = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    if not diff:
        return ''

    def name(r):
        return f"{r['kernel']}<{r['bm']},{r['bn']},mode {r['mode']}> splits {r['splits']} ({r['partial']})"
    return f'{case_id}: expected {name(want)}, the call ran {name(got)}; differing fields (got, expected): {diff}'


# ---- epilogue feature sets ---------------------------------------------------------------------------------------------------------
# pad: extra elements per row of the output (ldc = N + pad) and of the A / X operand; the residual and the row vector get another one
FEATS = {
    'plain':    dict(pad=0),
    'bias':     dict(bias=1, pad=8),
    'bias_res': dict(bias=1, res=1, pad=64),
    'bias_rv':  dict(bias=1, rv=1, pad=8),
    'all':      dict(bias=1, res=1, rv=1, pad=64),
    'f32':      dict(bias=1, res=1, f32=1, pad=8),
    'accum':    dict(bias=1, f32=1, accum=1, pad=64),
    'alpha':    dict(bias=1, res=1, alpha=0.5, pad=0),
    'alpha2':   dict(bias=1, alpha=2.0, pad=8),
    'silu':     dict(bias=1, silu=1, pad=8),
}
ALL_FEATS = tuple(FEATS)
NO_RV = tuple(f for f in FEATS if 'rv' not in FEATS[f])
AS_FEATS = ('plain', 'bias', 'bias_res', 'alpha')          # gemm_as_kernel: no row vector, no flags
BR_FEATS = ('plain', 'bias', 'f32_bias', 'silu')
FEATS['f32_bias'] = dict(bias=1, f32=1, pad=64)             # sidlsg_conv3x3_br_bf16: bias is its only epilogue operand
FEATS['f32_plain'] = dict(f32=1, pad=8)                     # the bare scaled accumulator (tests/test_gpu_fp8_bytes.py)


def feat_flags(f):
    return (OUT_F32 if f.get('f32') else 0) | (ACCUM if f.get('accum') else 0) | (SILU if f.get('silu') else 0)


def other_pad(pad):
    """A second padding, different from the output's, for the residual (elements; keeps 16-byte rows)."""
    return {0: 8, 8: 64, 64: 0}[pad]


# ---- the case tables ---------------------------------------------------------------------------------------------------------------
# rows_per_batch of the dense row-vector feature sets: >= 64 and no multiple of the tile height (two-vector path), < 16 * MT (per-element
# path), and M itself.
def rpb_values(M):
    return (100, 24, M)


# fp8: None (bf16 kernels), 'fp8w' (e4m3 weights, bf16 activations) or 'mx8' (both e4m3); sat: activations past +-448 (fp8w);
# small_ws: the workspace is set too small for two slabs for the call -> no split-K
def _dense(M, N, K, expect, feats=ALL_FEATS, p8=-1, g2=False, fp8=None, sat=False, small_ws=False):
    tag = f"{'-g2' if g2 else ''}{'-p8=%d' % p8 if p8 >= 0 else ''}{'-sat' if sat else ''}{'-smallws' if small_ws else ''}"
    return dict(ep='gemm', id=f"{fp8 or 'gemm'}-{M}x{N}x{K}{tag}", M=M, N=N, K=K, expect=expect, feats=feats, p8=p8, g2=g2, fp8=fp8, sat=sat, small_ws=small_ws)


def _conv(B, Hs, Ws, Cin, Cout, expect, stride=1, ups=0, feats=ALL_FEATS, g2=False, br=False, fp8=None, small_ws=False):
    tag = f"{'-s2' if stride == 2 else ''}{'-ups' if ups else ''}{'-br' if br else ''}{'-g2' if g2 else ''}{'-smallws' if small_ws else ''}"
    return dict(ep='conv_br' if br else 'conv', id=f"{fp8 + 'conv' if fp8 else 'conv'}-{B}x{Hs}x{Ws}x{Cin}-{Cout}{tag}", B=B, Hs=Hs, Ws=Ws, Cin=Cin, Cout=Cout,
                stride=2 if br else stride, ups=ups, expect=expect, feats=feats, g2=g2, p8=-1, fp8=fp8, sat=False, small_ws=small_ws)


GEMM_CASES = (
    # gemm_bf16_kernel<128, 64>: N <= 64; ragged N (element-wise epilogue), a K of one chunk
    _dense(200, 64, 72, rec('GEMM_BF16', 128, 64, 0, pad=1)),
    _dense(130, 12, 320, rec('GEMM_BF16', 128, 64, 0, pad=1)),
    _dense(65, 4, 8, rec('GEMM_BF16', 128, 64, 0, pad=1), feats=('plain', 'all', 'accum')),
    # <64, 64>: too few tiles for anything wider
    _dense(129, 136, 136, rec('GEMM_BF16', 64, 64, 0, pad=1)),
    _dense(65, 72, 8, rec('GEMM_BF16', 64, 64, 0, pad=1), feats=('plain', 'all', 'f32')),
    _dense(130, 136, 136, rec('GEMM_BF16', 64, 64, 0, pad=1), feats=('plain', 'all', 'f32'), g2=True),
    # <64, 128> from 384 tiles of 64 x 128, <128, 128> from 384 tiles of 128 x 128, <128, 128> split-K
    _dense(12300, 136, 72, rec('GEMM_BF16', 64, 128, 0, pad=1)),
    _dense(24600, 136, 72, rec('GEMM_BF16', 128, 128, 0, pad=1), feats=('plain', 'all', 'f32', 'accum')),
    _dense(300, 136, 4096, rec('GEMM_BF16', 128, 128, 0, splits=8, pad=1)),
    # <64, 160>: N % 160 == 0, fewer than 256 tiles of 128 x 160, K % 64 != 0 keeps the p8 rule out
    _dense(4100, 960, 72, rec('GEMM_BF16', 64, 160, 0, pad=1), feats=('plain', 'all', 'f32')),
    _dense(12300, 320, 72, rec('GEMM_BF16', 64, 160, 0, pad=1)),
    # gemm_v3_kernel: unsplit, with a K tail (K % 64 != 0), split-K
    _dense(16390, 320, 320, rec('GEMM_V3', 128, 160, 0)),
    _dense(12300, 640, 328, rec('GEMM_V3', 128, 160, 0), feats=('plain', 'all', 'f32', 'accum')),
    _dense(300, 640, 2560, rec('GEMM_V3', 128, 160, 0, splits=5)),
    _dense(16392, 320, 320, rec('GEMM_V3', 128, 160, 0), feats=('plain', 'all', 'f32'), g2=True),
    # the 256 x 320 kernel by the cost model, unsplit and split
    _dense(32770, 320, 320, rec('GEMM_P8W', 256, 320, 0, p8=1)),
    _dense(2100, 2560, 2560, rec('GEMM_P8W', 256, 320, 0, splits=3, p8=1), feats=('plain', 'all', 'f32')),
    # gemm_as_kernel: K = 320, N >= 2560, M >= 8192, no row vector, no flags
    _dense(8200, 2560, 320, rec('GEMM_AS', 128, 160, 0), feats=AS_FEATS),
    # both p8 configurations forced (sidlsg_debug_set_p8)
    _dense(20000, 160, 320, rec('GEMM_P8S', 256, 160, 0, p8=0), p8=1),
    _dense(16500, 320, 640, rec('GEMM_P8W', 256, 320, 0, p8=1), p8=2, feats=('plain', 'all', 'f32', 'accum')),
    _dense(1000, 320, 1536, rec('GEMM_P8S', 256, 160, 0, splits=2, p8=0), p8=1, feats=('plain', 'all', 'f32')),
    _dense(16502, 320, 640, rec('GEMM_P8W', 256, 320, 0, p8=1), p8=2, feats=('plain', 'all'), g2=True),
)

CONV_CASES = (
    # gemm_v3_kernel<1>, unsplit: 1296 rows per image are no multiple of the 128-row tile, so image boundaries fall inside tiles
    _conv(26, 36, 36, 64, 160, rec('GEMM_V3', 128, 160, 1)),
    _conv(26, 72, 72, 64, 160, rec('GEMM_V3', 128, 160, 1), stride=2, feats=('plain', 'all', 'f32')),
    _conv(26, 18, 18, 64, 160, rec('GEMM_V3', 128, 160, 1), ups=1, feats=('plain', 'all', 'f32')),
    _conv(26, 36, 36, 64, 160, rec('GEMM_V3', 128, 160, 1), feats=('plain', 'all'), g2=True),
    # the 256 x 320 kernel by the cost model
    _conv(9, 64, 64, 64, 320, rec('GEMM_P8W', 256, 320, 1, p8=1)),
    _conv(9, 128, 128, 64, 320, rec('GEMM_P8W', 256, 320, 1, p8=1), stride=2, feats=('plain', 'all', 'f32')),
    # gemm_bf16_kernel, any Cin (MODE 2) and Cin % 64 == 0 (MODE 1), every tile shape
    _conv(6, 64, 64, 8, 320, rec('GEMM_BF16', 128, 160, 2, pad=1)),
    _conv(4, 64, 64, 72, 320, rec('GEMM_BF16', 64, 160, 2, pad=1), feats=('plain', 'all', 'f32')),
    _conv(4, 64, 64, 8, 136, rec('GEMM_BF16', 64, 128, 2, pad=1), feats=('plain', 'all', 'f32')),
    _conv(12, 64, 64, 8, 136, rec('GEMM_BF16', 128, 128, 2, pad=1), feats=('plain', 'all', 'accum')),
    _conv(12, 64, 64, 64, 136, rec('GEMM_BF16', 128, 128, 1, pad=1)),
    _conv(4, 64, 64, 64, 136, rec('GEMM_BF16', 64, 128, 1, pad=1), feats=('plain', 'all', 'f32')),
    _conv(3, 9, 7, 72, 40, rec('GEMM_BF16', 128, 64, 2, pad=1), stride=2),
    _conv(2, 8, 8, 320, 8, rec('GEMM_BF16', 128, 64, 1, pad=1)),
    _conv(2, 12, 20, 8, 320, rec('GEMM_BF16', 64, 64, 2, pad=1)),
    _conv(2, 6, 10, 8, 320, rec('GEMM_BF16', 64, 64, 2, pad=1), ups=1, feats=('plain', 'all', 'f32')),
    _conv(4, 12, 20, 8, 320, rec('GEMM_BF16', 64, 64, 2, pad=1), feats=('plain', 'all'), g2=True),
    # split-K: v3 (N % 160 == 0, Cin % 64 == 0) and <128, 128, 2>
    _conv(2, 8, 8, 1280, 320, rec('GEMM_V3', 128, 160, 1, splits=15)),
    _conv(2, 8, 8, 232, 136, rec('GEMM_BF16', 128, 128, 2, splits=4, pad=1)),
    # pad = 'br' (bottom / right only, stride 2): its own entry point, PAD = 0 instantiations
    _conv(6, 128, 128, 64, 136, rec('GEMM_BF16', 128, 128, 1, pad=0), br=True, feats=BR_FEATS),
    _conv(2, 16, 16, 64, 128, rec('GEMM_BF16', 64, 64, 1, pad=0), br=True, feats=BR_FEATS),
    _conv(2, 16, 12, 72, 40, rec('GEMM_BF16', 64, 64, 2, pad=0), br=True, feats=BR_FEATS),
)


_F8W, _F8WC = rec('GEMM_FP8W', 128, 128, 0), rec('GEMM_FP8W', 128, 128, 2)

# gemm_fp8w_kernel: one 128 x 128 tile shape, 64-element K-tiles, no split-K
FP8W_CASES = (
    _dense(130, 24, 16, _F8W, fp8='fp8w'),                     # ragged N, K shorter than one K-tile
    _dense(200, 136, 80, _F8W, fp8='fp8w'),                    # K tail 64 + 16, N one tile and 8 columns
    _dense(129, 200, 144, _F8W, fp8='fp8w'),
    _dense(130, 136, 80, _F8W, fp8='fp8w', g2=True),           # halves of 65 rows: the second set starts mid-tile
    _dense(130, 136, 80, _F8W, fp8='fp8w', sat=True),          # activations past +-448 saturate in the loader
    _conv(3, 9, 7, 16, 40, _F8WC, stride=2, fp8='fp8w'),
    _conv(2, 6, 10, 48, 136, _F8WC, ups=1, fp8='fp8w'),
    _conv(2, 12, 20, 80, 136, _F8WC, fp8='fp8w'),              # Cin = 80: the taps straddle the 64-wide K-tile
    _conv(2, 12, 20, 80, 136, _F8WC, fp8='fp8w', g2=True),
)


def _mx(mode, splits=1):
    return rec('GEMM_MX8', 128, 160, mode, splits=splits)


# gemm_mx8_kernel: 128 x 160 tiles, 128-byte K-tiles; split-K from 16 K-tiles on (4 per split at least) while fewer than 384 tiles exist
MX8_CASES = (
    _dense(130, 160, 16, _mx(0), fp8='mx8'),                   # one 16-byte chunk
    _dense(300, 320, 144, _mx(0), fp8='mx8'),                  # K = 128 + 16
    _dense(129, 480, 320, _mx(0), fp8='mx8'),                  # three N tiles; tiles_m = 2 < group_m = 4
    _dense(700, 160, 128, _mx(0), fp8='mx8'),                  # six M tiles: a raster group of 4, then one of 2
    _dense(130, 160, 2048, _mx(0, 4), fp8='mx8'),              # nk = 16: 4 splits of 4
    _dense(130, 320, 2064, _mx(0, 4), fp8='mx8'),              # nk = 17 at 5 per split: 4 splits, the ragged chunk in the last one
    _dense(260, 160, 144, _mx(0), fp8='mx8', g2=True),
    _dense(260, 160, 2048, _mx(0, 4), fp8='mx8', g2=True),
    _conv(3, 9, 7, 16, 160, _mx(1), fp8='mx8'),
    _conv(2, 12, 20, 48, 160, _mx(1), fp8='mx8'),
    _conv(1, 10, 6, 144, 320, _mx(1, 4), fp8='mx8'),           # Cin = 128 + 16: nk = 18; the part-filled chunk of a tap runs into the next tap's weights
    _conv(2, 8, 8, 320, 160, _mx(1, 6), fp8='mx8'),            # nk = 27, one tile: 6 splits, the last one short
    _conv(1, 10, 6, 144, 320, _mx(1), fp8='mx8', small_ws=True),      # the unsplit K loop over all 18 / 27 K-tiles
    _conv(2, 8, 8, 320, 160, _mx(1), fp8='mx8', small_ws=True),
    _conv(4, 9, 7, 48, 160, _mx(1), fp8='mx8', g2=True),
)
FP8_CASES = FP8W_CASES + MX8_CASES

# wscale[n] = list[n % len]: exactly representable, and a period (7, 9) that divides none of 4, 8, 16, 80 -- a kernel that reads the scale
# of channel n + 4, n + 8, n + 16 or of the other wave's half (n + 80) changes the result
WSCALES = (0.25, 0.5, 1.0, 2.0, 3.0, 4.0, 6.0)
WSCALES1 = (2.0, 0.25, 6.0, 1.0, 3.0, 0.5, 4.0, 1.0, 0.5)
SAT_VALUES = (448.0, -448.0, 449.0, 1e4, -3e38)
MX8_SMALL_WS_BYTES = 64 << 10       # less than two slabs (M N 4 bytes each) of every `small_ws` forward row


def wscale_of(N, values):
    return torch.tensor(values, dtype=F32)[torch.arange(N) % len(values)]


def a_pad_of(c, pad):
    """Padding of the A / X operand (elements = bytes for mx8, where lda % 16 == 0 is required: 0, 16, 64)."""
    return {0: 0, 8: 16, 64: 64}[pad] if c.get('fp8') == 'mx8' else pad


def _wg(M, N, K, expect, **kw):
    return {**dict(ep='wgrad', id=f'wgrad-{M}x{N}x{K}' + ''.join(f'-{k}' for k in kw), M=M, N=N, K=K, expect=expect, small_ws=False, det=False), **kw}


def _wgc(B, Hs, Ws, Cin, Cout, expect, stride=1, ups=0, **kw):
    tag = f"{'-s2' if stride == 2 else ''}{'-ups' if ups else ''}" + ''.join(f'-{k}' for k in kw)
    return {**dict(ep='wgrad_conv', id=f'wgradconv-{B}x{Hs}x{Ws}x{Cin}-{Cout}{tag}', B=B, Hs=Hs, Ws=Ws, Cin=Cin, Cout=Cout, stride=stride, ups=ups,
                   expect=expect, small_ws=False, det=False), **kw}


# Weight gradients.  Every row runs accumulating and assigning (onto a NaN-filled dW), with a bias gradient.  `small_ws`: the workspace is
# set too small for two slabs for the call -> fp32 atomics; `det`: deterministic mode (the bias gradient through sidlsg_colsum).
WGRAD_CASES = (
    # wgrad_bf16_kernel: N % 8 != 0 (dense), Cout = 4 (conv_out)
    _wg(700, 12, 64, rec('WGRAD_BF16', 128, 128, 0, splits=3, partial='slabs')),
    _wg(100, 12, 64, rec('WGRAD_BF16', 128, 128, 0)),
    _wgc(2, 16, 16, 64, 4, rec('WGRAD_BF16', 128, 128, 1, splits=2, partial='slabs')),
    _wgc(1, 8, 8, 64, 4, rec('WGRAD_BF16', 128, 128, 1)),
    # wgrad_v2_kernel<0>
    _wg(512, 128, 128, rec('WGRAD_V2', 128, 128, 0, splits=2, partial='slabs')),
    _wg(200, 128, 128, rec('WGRAD_V2', 128, 128, 0)),
    _wg(777, 640, 640, rec('WGRAD_V2', 128, 128, 0, splits=4, partial='slabs')),
    # wgrad_v2s_kernel: N, K % 160 == 0, N != K, M >= 4096
    _wg(4100, 320, 160, rec('WGRAD_V2S', 160, 160, 0, splits=17, partial='slabs')),
    _wg(100, 5120, 1760, rec('WGRAD_V2S', 160, 160, 0)),          # (few rows: admitted by N K >= 8 Mi)
    # conv, by the constant-advance condition of launch_wgrad: v2f, v2wf, v2w<1>, v2<1>
    _wgc(2, 16, 16, 64, 128, rec('WGRAD_V2F', 128, 128, 1, splits=2, partial='slabs')),
    _wgc(1, 16, 8, 64, 128, rec('WGRAD_V2F', 128, 128, 1)),
    _wgc(1, 16, 16, 64, 320, rec('WGRAD_V2WF', 160, 128, 1)),
    _wgc(4, 16, 16, 64, 320, rec('WGRAD_V2WF', 160, 128, 1, splits=4, partial='slabs')),
    _wgc(2, 12, 20, 64, 320, rec('WGRAD_V2W', 160, 128, 1, splits=2, partial='slabs')),
    _wgc(1, 10, 20, 64, 320, rec('WGRAD_V2W', 160, 128, 1)),
    _wgc(2, 6, 10, 64, 320, rec('WGRAD_V2W', 160, 128, 1, splits=2, partial='slabs'), ups=1),
    _wgc(3, 9, 7, 72, 40, rec('WGRAD_V2', 128, 128, 1), stride=2),
    _wgc(12, 18, 14, 72, 40, rec('WGRAD_V2', 128, 128, 1, splits=3, partial='slabs'), stride=2),
    # the fp32-atomic fallback (no room for two slabs), and deterministic mode
    _wg(777, 640, 640, rec('WGRAD_V2', 128, 128, 0, splits=4, partial='atomics'), small_ws=True),
    _wgc(4, 16, 16, 64, 320, rec('WGRAD_V2WF', 160, 128, 1, splits=4, partial='atomics'), small_ws=True),
    _wg(777, 640, 640, rec('WGRAD_V2', 128, 128, 0, splits=4, partial='slabs', finish=FIN_REDUCE | FIN_COLSUM), det=True),
)

# Grouped dense weight gradients: ragged row counts, one job that assigns; (t160, [(M, N, K, assign)], expected record)
WGRAD_GROUPS = (
    dict(ep='wgrad_group', id='wgradgroup-128', t160=False, jobs=((777, 128, 320, 0), (300, 320, 128, 1), (1030, 136, 72, 0)),
         expect=rec('WGRAD_V2G', 128, 128, 0, splits=5, partial='slabs')),
    dict(ep='wgrad_group', id='wgradgroup-160', t160=True, jobs=((777, 320, 160, 0), (1030, 160, 320, 1), (300, 160, 160, 0)),
         expect=rec('WGRAD_V2SG', 160, 160, 0, splits=5, partial='slabs')),
)

ALL_CASES = GEMM_CASES + CONV_CASES + FP8W_CASES + MX8_CASES + WGRAD_CASES + WGRAD_GROUPS

# Kernel ids no row of the tables reaches, with the reason (tests/test_gemm_cases_host.py: every other id must appear)
UNREACHED = {
    'NONE': 'not a kernel: the record before the first launch',
    'GEMM_P8W_GEGLU': 'GEGLU fusion: gelu is not exact (out of scope)',
    'GEMM_P8W_GEGLU_BWD': 'GEGLU fusion: gelu is not exact (out of scope)',
}


def case_seed(c):
    """One seed per case: a fixed function of its id (never of anything measured)."""
    return 1 + sum((i + 1) * ord(ch) for i, ch in enumerate(c['id'])) % 100003


# ---- exact operands ----------------------------------------------------------------------------------------------------------------
def ints(gen, shape, lo, hi, dtype):
    """Integers in [lo, hi] as `dtype`; bf16 rounds what it cannot hold (to nearest even: still an integer); e4m3 holds every integer up to 16."""
    return torch.randint(lo, hi + 1, shape, generator=gen).to(F32).to(dtype)


def conv_geometry(c):
    """-> (H, W, Ho, Wo): the virtual (post-upsample) input size and the output size."""
    H, W = (2 * c['Hs'], 2 * c['Ws']) if c['ups'] else (c['Hs'], c['Ws'])
    if c['ep'] == 'conv_br':
        return H, W, H // 2, W // 2
    return H, W, (H - 1) // c['stride'] + 1, (W - 1) // c['stride'] + 1


def mnk(c):
    """-> (M, N, K) of the contraction a case runs (conv: output pixels, Cout, 9 Cin)."""
    if c['ep'] in ('gemm', 'wgrad'):
        return c['M'], c['N'], c['K']
    _, _, Ho, Wo = conv_geometry(c)
    return c['B'] * Ho * Wo, c['Cout'], 9 * c['Cin']


def fwd_operands(c):
    """The logical operands of a forward case: a / x, w (w1), bias (bias1), rv, res, cprev -- CPU tensors, never modified by a caller."""
    g = torch.Generator().manual_seed(case_seed(c))
    M, N, K = mnk(c)
    fp8 = c.get('fp8')
    adt, wdt = (F8 if fp8 == 'mx8' else BF16), (F8 if fp8 else BF16)
    o = {}
    if c['ep'] == 'gemm':
        o['a'] = ints(g, (M, K), -3, 3, adt)
        nb = {r: (M + r - 1) // r for r in rpb_values(M)}
    else:
        o['a'] = ints(g, (c['B'], c['Hs'], c['Ws'], c['Cin']), -3, 3, adt)
        nb = {M // c['B']: c['B']}
    if c.get('sat'):             # about 1 % of the entries past (or at) the e4m3 range
        hit = torch.rand(o['a'].shape, generator=g) < 0.01
        o['a'] = torch.where(hit, torch.tensor(SAT_VALUES)[torch.randint(0, len(SAT_VALUES), o['a'].shape, generator=g)].to(BF16), o['a'])
    o['w'] = ints(g, (N, K), -2, 2, wdt)
    o['bias'] = ints(g, (N,), -1000, 1000, F32)
    if fp8:
        o['wscale'] = wscale_of(N, WSCALES)
    if c['g2']:
        o['w1'] = ints(g, (N, K), -2, 2, wdt)
        o['bias1'] = ints(g, (N,), -1000, 1000, F32)
        if fp8:
            o['wscale1'] = wscale_of(N, WSCALES1)
    o['rv'] = {r: ints(g, (n, N), -300, 300, F32) for r, n in nb.items()}
    o['res'] = ints(g, (M, N), -1000, 1000, BF16)
    o['cprev'] = ints(g, (M, N), -1000, 1000, F32)
    return o


def wgrad_operands(c):
    g = torch.Generator().manual_seed(case_seed(c))
    M, N, K = mnk(c)
    a = ints(g, (M, K), -3, 3, BF16) if c['ep'] == 'wgrad' else ints(g, (c['B'], c['Hs'], c['Ws'], c['Cin']), -3, 3, BF16)
    return dict(a=a, dy=ints(g, (M, N), -3, 3, BF16), dw_prev=ints(g, (N, K), -1000, 1000, F32), db_prev=ints(g, (N,), -1000, 1000, F32))


# ---- references (fp64; every value is an integer or a half, so fp64 holds it exactly) ----------------------------------------------
def conv_taps(x, stride, ups, br=False):
    """x [B, Hs, Ws, C] -> the nine shifted views [B, Ho, Wo, C] (fp64) a 3x3 window reads, tap-major (dh * 3 + dw): pad 1 on all four sides,
    or (br) zero padding on the bottom and right only with stride 2; `ups` reads x through a nearest x2 upsample."""
    x = x.float().to(F64)
    if ups:
        x = x.repeat_interleave(2, 1).repeat_interleave(2, 2)
    B, H, W, C = x.shape
    if br:
        xp, Ho, Wo, stride = F.pad(x, (0, 0, 0, 1, 0, 1)), H // 2, W // 2, 2
    else:
        xp, Ho, Wo = F.pad(x, (0, 0, 1, 1, 1, 1)), (H - 1) // stride + 1, (W - 1) // stride + 1
    return [xp[:, dh:dh + stride * (Ho - 1) + 1:stride, dw:dw + stride * (Wo - 1) + 1:stride, :] for dh in range(3) for dw in range(3)]


def contract(c, a, w):
    """A W^T in fp64 -> [M, N]: dense rows, or the 3x3 conv as nine per-tap products (w: [N][9 Cin], tap-major like the kernels' weights)."""
    a, w = a.float(), w.float()          # (exact: bf16 and e4m3 values are fp32 values)
    if c.get('fp8') == 'fp8w':           # the loader's saturating conversion; the identity on the integers of every row but `sat`
        a = a.clamp(-448, 448)
    if c['ep'] == 'gemm':
        return a.to(F64) @ w.to(F64).t()
    Cin = c['Cin']
    acc = None
    for t, v in enumerate(conv_taps(a, c['stride'], c['ups'], c['ep'] == 'conv_br')):
        part = v.reshape(-1, Cin) @ w[:, t * Cin:(t + 1) * Cin].to(F64).t()
        acc = part if acc is None else acc + part
    return acc


@functools.lru_cache(maxsize=4)
def _accumulators(case_id):
    c = next(x for x in ALL_CASES if x['id'] == case_id)
    o = fwd_operands(c)
    M = mnk(c)[0]
    acc = contract(c, o['a'], o['w'])
    if c.get('fp8'):
        acc = acc * o['wscale'].to(F64)
    if c['g2']:              # rows (samples) of the second half with the second weight set
        acc1 = contract(c, o['a'], o['w1'])
        if c.get('fp8'):
            acc1 = acc1 * o['wscale1'].to(F64)
        acc = torch.cat([acc[:M // 2], acc1[M // 2:]])
    return o, acc


def fwd_reference(c, feat, rpb=None):
    """-> (operands, exact fp64 result [M, N] BEFORE the output rounding) of feature set `feat` (a FEATS key); e4m3 rows: the accumulator
    is wscale[n] * acc."""
    f = FEATS[feat]
    o, acc = _accumulators(c['id'])
    M, N, _ = mnk(c)
    x = acc * f.get('alpha', 1.0)
    if f.get('bias'):
        b = o['bias'].to(F64).expand(M, N)
        if c['g2']:
            b = torch.cat([b[:M // 2], o['bias1'].to(F64).expand(M, N)[M // 2:]])
        x = x + b
    if f.get('rv'):
        x = x + o['rv'][rpb].to(F64)[torch.arange(M) // rpb]
    if f.get('res'):
        x = x + o['res'].to(F64)
    if f.get('silu'):
        x = x * torch.sigmoid(x)
    if f.get('accum'):
        x = x + o['cprev'].to(F64)
    return o, x


def round_out(x64, dtype):
    """The one rounding a correct kernel applies: fp64 -> fp32 is exact for these values, fp32 -> bf16 rounds to nearest even."""
    x32 = x64.to(F32)
    assert torch.equal(x32.to(F64), x64), 'reference value is not exact in fp32'
    return x32 if dtype == F32 else x32.to(BF16)


def wgrad_reference(c, o):
    """-> (dW [N, K], dB [N]) in fp64, WITHOUT the previous contents."""
    dy = o['dy'].to(F64)
    if c['ep'] == 'wgrad':
        return dy.t() @ o['a'].to(F64), dy.sum(0)
    Cin = c['Cin']
    return torch.cat([dy.t() @ v.reshape(-1, Cin) for v in conv_taps(o['a'], c['stride'], c['ups'])], 1), dy.sum(0)


def transpose_taps(w, Cout, Cin):
    """[Cout][9][Cin] -> [Cin][9 reversed][Cout]: the backward-data operand sidlsg_transpose_w makes."""
    return w.view(Cout, 9, Cin).flip(1).permute(2, 1, 0).reshape(Cin, 9 * Cout).contiguous()


def dgrad_reference(dy, w, x_shape, stride, ups):
    """The data gradient of conv3x3 as ops._conv_dgrad forms it, with its bf16 rounding points: (stride 2) dy zero-inserted to the input's size,
    a pad-1 conv with the transposed, tap-flipped weights rounded to bf16, (ups) the four full-resolution gradients of an input pixel summed and
    rounded to bf16 again.  dy [B, Ho, Wo, Cout] bf16, w [Cout][9 Cin] bf16 -> dx bf16 of x_shape (the SOURCE size under ups)."""
    B, Hs, Ws, Cin = x_shape
    Cout = dy.shape[3]
    H, W = (2 * Hs, 2 * Ws) if ups else (Hs, Ws)
    g = dy.to(F64)
    if stride == 2:
        z = torch.zeros(B, H, W, Cout, dtype=F64)
        z[:, ::2, ::2][:, :dy.shape[1], :dy.shape[2]] = g
        g = z
    wt = transpose_taps(w, Cout, Cin).to(F64)
    full = sum(v.reshape(-1, Cout) @ wt[:, t * Cout:(t + 1) * Cout].t() for t, v in enumerate(conv_taps(g, 1, 0))).view(B, H, W, Cin)
    full = round_out(full, BF16)
    if not ups:
        return full
    return round_out(full.to(F64).view(B, Hs, 2, Ws, 2, Cin).sum(dim=(2, 4)), BF16)


# ---- judging a result --------------------------------------------------------------------------------------------------------------
def bits(t):
    return t.contiguous().view(INT_OF[t.dtype])


def _low16(x64):
    """The 16 bits of the fp32 form of x (exact for these values: round_out asserts it) that a bf16 drops."""
    return x64.to(F32).contiguous().view(torch.int32) & 0xFFFF


def needs_rounding(x64):
    """Per element: does x need rounding to become bf16?"""
    return _low16(x64) != 0


def is_tie(x64):
    """Per element: x lies exactly half way between two neighbouring bf16 values."""
    return _low16(x64) == 0x8000


def tie_goes_up(x64):
    """Per element, meaningful where is_tie: nearest-even moves a tie away from zero iff the kept mantissa is odd."""
    return ((x64.to(F32).contiguous().view(torch.int32) >> 16) & 1) == 1


def truncate_bf16(x32):
    """fp32 -> bf16 by dropping the low 16 bits: the wrong rounding mode a mutant uses."""
    return (x32.contiguous().view(torch.int32) >> 16).to(torch.int16).view(BF16)


def exact_mismatch(got, want):
    """'' when `got` equals `want` bit for bit (same dtype and shape), else a message with the count and the first differing element."""
    assert got.dtype == want.dtype and got.shape == want.shape, f'{got.dtype} {tuple(got.shape)} vs {want.dtype} {tuple(want.shape)}'
    if torch.isnan(got.float()).any():
        return f'{int(torch.isnan(got.float()).sum())} NaN in the output'
    bad = bits(got) != bits(want)
    if not bad.any():
        return ''
    idx = tuple(int(i) for i in bad.nonzero()[0])
    return f'{int(bad.sum())} of {bad.numel()} elements differ; first at {idx}: got {got[idx].item()}, expected {want[idx].item()}'


def silu_mismatch(got, want64):
    g = got.double()
    if not torch.isfinite(g).all():
        return 'non-finite output'
    err = ((g - want64).abs().max() / want64.abs().max()).item()
    return '' if err < SILU_TOL else f'rel max err {err:.3e} (tol {SILU_TOL})'


# ---- guarded and poisoned buffers --------------------------------------------------------------------------------------------------
def guarded(rows, cols, pad, dtype, device, fill=None):
    """-> (whole, view): `whole` has rows + GUARD rows of cols + pad elements, every element the sentinel; `view` = whole[:rows, :cols] is what
    the kernel gets (pointer view.data_ptr(), row stride cols + pad), filled from `fill` ([rows, cols]) when given."""
    whole = torch.full((rows + GUARD, cols + pad), SENTINEL[dtype], dtype=INT_OF[dtype], device=device).view(dtype)
    view = whole[:rows, :cols]
    if fill is not None:
        view.copy_(fill.to(device=device, dtype=dtype))
    return whole, view


def guard_damage(whole, rows, cols):
    """'' when every element of `whole` outside [0, rows) x [0, cols) still holds the sentinel, else where the first damage is."""
    b = bits(whole) != SENTINEL[whole.dtype]
    b[:rows, :cols] = False
    if not b.any():
        return ''
    r, col = (int(i) for i in b.nonzero()[0])
    return f'{int(b.sum())} guard elements overwritten; first at row {r}, column {col} (the output is {rows} x {cols})'


def poisoned(t2d, pad, device):
    """An input [rows, cols] as the kernel reads it: row stride cols + pad, NaN in the padding columns and in GUARD rows after the last row.
    -> the view [rows, cols] (pointer .data_ptr(), stride .stride(0))."""
    rows, cols = t2d.shape
    if t2d.dtype == F8:          # (bytes: e4m3 tensors have no fill / copy kernels of their own everywhere)
        whole = torch.full((rows + GUARD, cols + pad), SENTINEL[F8], dtype=torch.uint8, device=device)
        whole[:rows, :cols] = t2d.contiguous().view(torch.uint8).to(device)
        return whole.view(F8)[:rows, :cols]
    whole = torch.full((rows + GUARD, cols + pad), float('nan'), dtype=t2d.dtype, device=device)
    whole[:rows, :cols] = t2d.to(device)
    return whole[:rows, :cols]


def poisoned_flat(t, device, dtype=None):
    """A contiguous operand followed by GUARD * 8 sentinel elements -> (whole, view of the operand's shape)."""
    dtype = dtype or t.dtype
    n = t.numel()
    whole = torch.full((n + GUARD * 8,), SENTINEL[dtype], dtype=INT_OF[dtype], device=device)
    if dtype == F8:
        whole[:n] = t.reshape(-1).view(torch.uint8).to(device)
        whole = whole.view(dtype)
    else:
        whole = whole.view(dtype)
        whole[:n] = t.reshape(-1).to(device=device, dtype=dtype)
    return whole, whole[:n].view(t.shape)


def flat_damage(whole, n):
    b = bits(whole[n:]) != SENTINEL[whole.dtype]
    return '' if not b.any() else f'{int(b.sum())} guard elements after the operand overwritten; first at offset {n + int(b.nonzero()[0])}'


# ---- the calls ---------------------------------------------------------------------------------------------------------------------
def fwd_layout(c, feat):
    """Row strides of a forward call's operands (elements): shared by the GPU run and the no-GPU dispatch check, so both see one call."""
    f = FEATS[feat]
    M, N, K = mnk(c)
    pad = f['pad']
    inner = K if c['ep'] == 'gemm' else c['Cin']
    return dict(lda=inner + a_pad_of(c, pad), ldc=N + pad, ldres=N + other_pad(pad), ldrv=N + pad)


def fwd_call(c, feat, rpb, p):
    """-> (entry point name, argument list).  p: addresses a, w, w1, c, bias, bias1, res, rv, stream (None where the feature set has none); e4m3
    rows also wscale, wscale1: every weight pointer is followed by its scale vector."""
    f = FEATS[feat]
    M, N, K = mnk(c)
    L = fwd_layout(c, feat)
    g2 = c['g2']
    bias = (p['bias'], p['bias1']) if g2 else (p['bias'],)
    if not f.get('bias'):
        bias = (None,) * len(bias)
    w = (p['w'], p['w1']) if g2 else (p['w'],)
    fp8 = c.get('fp8')
    if fp8:
        w = (p['w'], p['wscale'], p['w1'], p['wscale1']) if g2 else (p['w'], p['wscale'])
    sfx = f"_{fp8 or 'bf16'}{'_g2' if g2 else ''}"
    res, rv = (p['res'] if f.get('res') else None), (p['rv'] if f.get('rv') else None)
    if c['ep'] == 'gemm':
        return ('sidlsg_gemm' + sfx,
                [p['a'], L['lda'], *w, p['c'], L['ldc'], *bias, res, L['ldres'] if res else 0, rv, L['ldrv'] if rv else 0, rpb or 1, M, N, K,
                 float(f.get('alpha', 1.0)), feat_flags(f), p['stream']])
    H, W, _, _ = conv_geometry(c)
    if c['ep'] == 'conv_br':
        return 'sidlsg_conv3x3_br_bf16', [p['a'], L['lda'], p['w'], p['c'], L['ldc'], bias[0], c['B'], H, W, c['Cin'], c['Cout'], feat_flags(f), p['stream']]
    geom = () if fp8 == 'mx8' else (c['stride'], c['ups'])          # sidlsg_conv3x3_mx8: stride 1, no upsampling
    return ('sidlsg_conv3x3' + sfx,
            [p['a'], L['lda'], *w, p['c'], L['ldc'], *bias, res, L['ldres'] if res else 0, rv, L['ldrv'] if rv else 0, c['B'], H, W, c['Cin'], c['Cout'],
             *geom, float(f.get('alpha', 1.0)), feat_flags(f), p['stream']])


def fwd_runs(c):
    """-> [(feature set, rows_per_batch or None)]: every call a forward row makes."""
    out = []
    for feat in c['feats']:
        if FEATS[feat].get('rv'):
            out += [(feat, r) for r in (rpb_values(c['M']) if c['ep'] == 'gemm' else (mnk(c)[0] // c['B'],))]
        else:
            out.append((feat, None))
    return out


WG_PAD_Y, WG_PAD_A = 8, 64          # padding columns of dY and A / X in the weight-gradient calls


def wgrad_call(c, assign, p):
    """p: addresses dy, a, dw, db, stream."""
    M, N, K = mnk(c)
    if c['ep'] == 'wgrad':
        return ('sidlsg_wgrad_assign_bf16' if assign else 'sidlsg_wgrad_bf16', [p['dy'], N + WG_PAD_Y, p['a'], K + WG_PAD_A, p['dw'], p['db'], M, N, K, p['stream']])
    H, W, _, _ = conv_geometry(c)
    return ('sidlsg_conv3x3_wgrad_assign_bf16' if assign else 'sidlsg_conv3x3_wgrad_bf16',
            [p['dy'], N + WG_PAD_Y, p['a'], c['Cin'] + WG_PAD_A, p['dw'], p['db'], c['B'], H, W, c['Cin'], c['Cout'], c['stride'], c['ups'], p['stream']])


SMALL_WS_BYTES = 1 << 20            # less than two slabs of every `small_ws` row (N K 4 bytes each)


class WgJob(ctypes.Structure):
    _fields_ = [('dY', ctypes.c_void_p), ('A', ctypes.c_void_p), ('dW', ctypes.c_void_p), ('dBias', ctypes.c_void_p), ('ldy', ctypes.c_int),
                ('lda', ctypes.c_int), ('M', ctypes.c_int), ('N', ctypes.c_int), ('K', ctypes.c_int), ('assign', ctypes.c_int), ('pad', ctypes.c_int * 2)]


def group_jobs(c, ptrs):
    """The host records of a grouped weight gradient; ptrs: per job (dy, a, dw, db) addresses."""
    arr = (WgJob * len(c['jobs']))()
    for r, (M, N, K, assign), (dy, a, dw, db) in zip(arr, c['jobs'], ptrs):
        r.dY, r.A, r.dW, r.dBias, r.ldy, r.lda, r.M, r.N, r.K, r.assign = dy, a, dw, db, N + WG_PAD_Y, K + WG_PAD_A, M, N, K, assign
    return arr


def group_operands(c):
    g = torch.Generator().manual_seed(case_seed(c))
    return [dict(a=ints(g, (M, K), -3, 3, BF16), dy=ints(g, (M, N), -3, 3, BF16), dw_prev=ints(g, (N, K), -1000, 1000, F32),
                 db_prev=ints(g, (N,), -1000, 1000, F32)) for M, N, K, _ in c['jobs']]
