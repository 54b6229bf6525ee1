"""Shared by tests/test_elementwise_cases_host.py and tests/test_gpu_elementwise_edges.py (not a test module): case tables, input
builders, fp64 references, fp32 CPU emulations of the fast formulas, the metrics and MUTATIONS for the kernels of
sid_lsg_amd/csrc/elementwise.hip and optim.hip -- the activations, GEGLU, the layout ops, colsum, the SiD losses, the fused
Adam / EMA step, the weight-preparation casts and transposes, the timestep embedding.

Guard zones.  Every output of a GPU test is a view into a larger buffer (Guarded) whose other elements hold a sentinel bit pattern, a
NaN with a payload no kernel produces (bf16 0x7fc1, fp32 0x7fc12345), GUARD = 64 elements on each side.  After the call the guards
must be bit-unchanged and no element of the extent may still hold the sentinel; where the contract is `+=` the extent is pre-filled
with known values.

Exact inputs.  The sums (colsum, sumpool2x2, add) get non-zero integers of [-8, 8]: exact in bf16, every partial sum stays below
2^24 and so is exact in fp32 in any order (the host test asserts it per case); the check is torch.equal with the fp64 sum.

Activation sweep.  x = every one of the 65,536 bf16 bit patterns in a fixed shuffled order (so that a non-finite input shares its
8-vector with finite ones); the fp32 kernels get these widened plus 65,536 random finite fp32 patterns.  fp64 reference: SiLU by the
sigmoid, GELU x Phi(x) with Phi = erfc(-x / sqrt 2) / 2 (the erf form without the cancellation of 1 + erf in the left tail).
Bound per element, bf16 kernels: |got - ref| <= ulp_bf16(ref) + A -- one ulp, not a half, because an fp32 error of 1e-7 relative
can move a tie; ulp_bf16 is the bf16 spacing at ref (2^-133 below the smallest normal).  fp32 kernels: 2e-5 |ref| + A_f32 (2e-5:
the bound of tests/test_gpu_fp32.py, here per element).  Where |ref| exceeds the largest finite output the infinity of that sign is
accepted as well.  Only non-finite x is left out (256 patterns, NONFINITE_CAP = 0.5 % of a sweep); a NaN input must give NaN.

A is the ABSOLUTE part of the error the formulas have before the final rounding: `python tests/elementwise_cases.py` evaluates
gelu_fast / sigmoid_fast / silu_grad_t<bf16> (and silu_f / gelu_f / gelu_grad_f for A_f32) in fp32 on the CPU over the sweep and
takes a = max(|f - ref| - REL |ref|, 0): an fp32 formula also has an error RELATIVE to its value (|x| 2^-24 through the exponential
of a large argument, 5e-6 at x = -80), which the ulp term absorbs -- REL = 2^-16 is 1/256 of a bf16 ulp -- and which would make a
plain maximum of |f - ref| over a sweep that reaches 3e38 meaningless; for the fp32 kernels REL is the 2e-5 of the bound itself.
A = max(2 a, 1e-6) (the floor: a handful of 2^-23 relative errors on O(1) terms, the hardware's exp2 / rcp are 1 ulp and need not
agree with the CPU's).  profiles/elementwise_tolerance.txt has the table per kernel and input variant; the largest a is 4.6e-7
(geglu_bwd, randn value half and dy; 2.1e-7 where both are 1: the Abramowitz-Stegun erf of common.h, 5.4e-7 on erf, at gelu values
too small for the relative term; SiLU stays at 3e-37, its flush to zero below x = -88.7), so the derived value is the floor for all:
    A_BF16 = 1e-6        A_F32 = 1e-6  (largest a 2.8e-7, geglu_fwd randn)

Losses.  Reference: oracle/sid_ref.py on .double() inputs; value 1e-5 relative, gradients 1e-5 of the maximum WITHIN each sample
(w differs per sample), a dropped sample's gradient exactly 0.  g_loss_ref64 restates the generator loss in closed form only to
carry the mutations; the host test pins it to sid_ref.  Optimizer: sid_ref.adam_step_ref / torch.optim at the bounds of
tests/test_gpu_ops.py (1e-6 and 2e-6 of the maximum), taken over the ordinary elements and over the NaN / inf ones separately.

Measured on the MI355X (tests/test_gpu_elementwise_edges.py, largest |err| / bound; MEASURED_MI355X below): every bf16 activation
kernel 0.500 -- the half ulp of a correct rounding, i.e. the fast forms and the A-S tail never leave the nearest or second-nearest
bf16 number; fp32 activations at most 0.21 (geglu_bwd), timestep embedding 0.16 (bf16) / 0.27 (fp32), the losses at most 0.043, the
optimizer 0.20 (exp_avg_sq), 0.17 (p), 0.14 (exp_avg), 0.12 (ema).  colsum, the layout ops, the casts and the transposes are exact.
Before the optimizer kernel took 1 - beta2 from the host, exp_avg_sq stood at 13x its bound (1.f - 0.999f is 1.3e-5 off 0.001f).
"""
import collections
import math
import os

import numpy as np
import torch

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
GUARD = 64
SENTINEL = {BF16: 0x7fc1, F32: 0x7fc12345}
BITS = {BF16: torch.int16, F32: torch.int32}
OUT_MAX = {BF16: float(torch.finfo(BF16).max), F32: float(torch.finfo(F32).max)}
EINVAL = -22

# largest err / bound of tests/test_gpu_elementwise_edges.py on an MI355X (pytest -s prints them)
MEASURED_MI355X = {
    'silu_fwd bf16': 0.500, 'silu_bwd bf16': 0.500, 'geglu_fwd bf16': 0.500, 'geglu_bwd bf16': 0.500, 'geglu_bwd gate bf16': 0.500,
    'silu_fwd f32': 0.010, 'silu_bwd f32': 0.047, 'geglu_fwd f32': 0.196, 'geglu_bwd f32': 0.211, 'geglu_bwd gate f32': 0.045,
    'timestep_embed bf16': 0.163, 'timestep_embed f32': 0.265, 'g_loss': 0.037, 'fake_loss': 0.012, 'fake_loss_v': 0.043,
    'adam p': 0.167, 'adam ema': 0.115, 'adam exp_avg': 0.143, 'adam exp_avg_sq': 0.202, 'adam p vs torch.optim': 0.015,
}


# ---- guard zones -------------------------------------------------------------------------------------------------------------------
class Guarded:
    """A tensor `t` of `shape` inside a sentinel-filled buffer: GUARD elements (plus `shift`) in front, GUARD behind."""

    def __init__(self, shape, dtype, device, fill=None, shift=0):
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        n = int(np.prod(shape))
        total = (GUARD + shift + n + GUARD + 7) // 8 * 8
        self.dtype, self.n, self.lo = dtype, n, GUARD + shift
        self.buf = torch.full((total,), SENTINEL[dtype], dtype=BITS[dtype], device=device).view(dtype)
        self.t = self.buf[self.lo:self.lo + n].view(shape)
        if fill is not None:
            self.t.copy_(fill.to(dtype).view(shape) if torch.is_tensor(fill) else torch.full(shape, fill, dtype=dtype))
        self.before = self.bits().clone() if fill is not None else None

    def bits(self):
        return self.buf.view(BITS[self.dtype])

    def ptr(self):
        return self.t.data_ptr()

    def guards_intact(self):
        b = self.bits()
        return bool((b[:self.lo] == SENTINEL[self.dtype]).all()) and bool((b[self.lo + self.n:] == SENTINEL[self.dtype]).all())

    def all_written(self, allow=None):
        """No element still holds the sentinel; `allow` (bool, t's shape) exempts elements whose expected value is a NaN that came from
        the input -- the hardware hands a NaN's payload on, and the input sweeps hold every payload, the sentinel's too."""
        stale = self.bits()[self.lo:self.lo + self.n] == SENTINEL[self.dtype]
        if allow is not None:
            stale &= ~allow.to(stale.device).flatten()
        return not bool(stale.any())

    def untouched(self):
        """Nothing of the buffer changed since construction (a refused call; a source that must stay as it was)."""
        ref = self.before if self.before is not None else torch.full_like(self.bits(), SENTINEL[self.dtype])
        return torch.equal(self.bits(), ref)

    def check(self, name='', written=True, allow=None):
        assert self.guards_intact(), f'{name}: a write outside the output\'s extent (guard zone changed)'
        if written:
            assert self.all_written(allow), f'{name}: elements of the output were never written'
        return self.t


def bits_equal(a, b):
    """Bit for bit, NaNs and the sign of zero included."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(BITS[a.dtype]).cpu(), b.contiguous().view(BITS[b.dtype]).cpu())


def int_values(shape, seed, dtype=F32):
    """Non-zero integers of [-8, 8]."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(1, 9, tuple(shape), generator=g) * (torch.randint(0, 2, tuple(shape), generator=g) * 2 - 1)
    return v.to(dtype)


def distinct_values(n, dtype, start=0):
    """n different finite values: consecutive positive bf16 bit patterns, or integers."""
    if dtype == BF16:
        assert 0x80 + start + n < 0x7f80
        return torch.arange(0x80 + start, 0x80 + start + n, dtype=torch.int16).view(BF16)
    return torch.arange(1 + start, 1 + start + n, dtype=F32)


def randn_bf16(n, seed, scale=1.0):
    return (torch.randn(n, generator=torch.Generator().manual_seed(seed)) * scale).to(BF16)


# ---- activations -------------------------------------------------------------------------------------------------------------------
REL_BF16 = 2.0 ** -16        # relative fp32 error the ulp term absorbs (module docstring)
REL_F32 = 2e-5               # tests/test_gpu_fp32.py
A_FLOOR = 1e-6
NONFINITE_CAP = 0.005
ACT_OPS = ('silu_fwd', 'silu_bwd', 'geglu_fwd', 'geglu_bwd')
ACT_VARIANTS = ('ones', 'randn')
A_BF16 = 1e-6                # max(2 a, A_FLOOR) over every op and input variant: the floor (profiles/elementwise_tolerance.txt)
A_F32 = 1e-6
A_OF = {BF16: A_BF16, F32: A_F32}
SWEEP_F = 512                # the sweep as a GEGLU gate: [n / 512][512]

SILU_N = (8, 8 * 255, 8 * 256, 8 * 257)
GEGLU_MF = ((1, 8), (7, 24), (257, 8), (33, 640))
CONCAT_CASES = ((1, 8, 8), (35, 8, 24), (35, 320, 8), (70, 64, 32))
SUMPOOL_CASES = ((1, 1, 1, 8), (3, 5, 7, 24), (2, 4, 4, 320))
ZERO_INSERT_HW = ((1, 1), (7, 8), (8, 7), (9, 9))
ZERO_INSERT_C, ZERO_INSERT_B = (8, 24), 3


def sweep_x(dtype):
    """Every bf16 bit pattern in a fixed shuffled order (+ 65,536 random finite fp32 patterns for the fp32 kernels)."""
    g = torch.Generator().manual_seed(20240)
    pat = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16)[torch.randperm(65536, generator=g)].view(BF16)
    if dtype == BF16:
        return pat
    w = torch.randint(-2 ** 31, 2 ** 31, (65536,), generator=g, dtype=torch.int64).to(torch.int32)
    w = torch.where((w >> 23) & 0xff == 0xff, w & ~(1 << 23), w)           # exponent 255 -> 254: finite
    return torch.cat([pat.float(), w.view(F32)])[torch.randperm(131072, generator=g)]


def sweep_inputs(op, variant, dtype):
    """-> dict(x, a, dy): a (GEGLU value half) and dy as the op needs them, of `dtype`."""
    x = sweep_x(dtype)
    n = x.numel()
    mk = lambda seed: torch.ones(n, dtype=dtype) if variant == 'ones' else randn_bf16(n, seed).to(dtype)  # noqa: E731
    return dict(x=x, a=mk(11) if op.startswith('geglu') else None, dy=mk(12) if op.endswith('bwd') else None)


def _phi64(x):
    return 0.5 * torch.special.erfc(-x * math.sqrt(0.5))


def _gelu64(x, mutation=None):
    if mutation == 'tanh_gelu':
        return 0.5 * x * (1 + torch.tanh(math.sqrt(2 / math.pi) * (x + 0.044715 * x ** 3)))
    if mutation == 'sigmoid_gelu':
        return x * torch.sigmoid(1.702 * x)
    return x * _phi64(x)


def act_ref64(op, x, a=None, dy=None, mutation=None):
    """fp64 reference -> tuple of outputs (geglu_bwd: d value half, d gate half)."""
    x = x.double()
    a = None if a is None else a.double()
    dy = None if dy is None else dy.double()
    if op == 'silu_fwd':
        return (x * torch.sigmoid(x),)
    if op == 'silu_bwd':
        s = torch.sigmoid(x)
        return (dy * (s if mutation == 'silu_grad_no_x' else s * (1 + x * (1 - s))),)
    if op == 'geglu_fwd':
        return (a * _gelu64(x, mutation),)
    if mutation in ('tanh_gelu', 'sigmoid_gelu'):
        xr = x.clone().requires_grad_()
        gd, = torch.autograd.grad(_gelu64(xr, mutation).sum(), xr)
    else:
        gd = _phi64(x) + x * math.sqrt(0.5 / math.pi) * torch.exp(-0.5 * x * x)
    return (dy * _gelu64(x, mutation), dy * a * gd)


def _sigmoid_fast(x):
    return 1.0 / (1.0 + torch.exp2(-1.4426950408889634 * x))


def _gelu_fast(x):
    ax = x.abs() * 0.70710678118654752
    t = 1.0 / (0.3275911 * ax + 1.0)
    p = 1.061405429 * t - 1.453152027
    p = p * t + 1.421413741
    p = p * t - 0.284496736
    p = p * t + 0.254829592
    e = torch.exp2(-0.72134752044448170 * x * x)
    erfv = torch.copysign(1.0 - p * t * e, x)
    cdf = 0.5 * erfv + 0.5
    return x * cdf, x * 0.3989422804014327 * e + cdf


def act_emulated(op, x, a=None, dy=None, dtype=BF16):
    """The kernels' formulas (common.h: the fast forms for bf16 storage, the erff / division forms for fp32) in fp32 on the CPU,
    BEFORE the final rounding to the storage type."""
    x = x.float()
    a = None if a is None else a.float()
    dy = None if dy is None else dy.float()
    fast = dtype == BF16
    if op.startswith('silu'):
        s = _sigmoid_fast(x) if fast else 1.0 / (1.0 + torch.exp(-x))
        if op == 'silu_fwd':
            return (x * s if fast else x / (1.0 + torch.exp(-x)),)
        return (dy * (s * (x * (1.0 - s) + 1.0)),)
    if fast:
        gl, gd = _gelu_fast(x)
    else:
        cdf = 0.5 * (1.0 + torch.erf(x * 0.70710678118654752))
        gl, gd = 0.5 * x * (1.0 + torch.erf(x * 0.70710678118654752)), cdf + x * (0.3989422804014327 * torch.exp(-0.5 * x * x))
    if op == 'geglu_fwd':
        return (a * gl,)
    return (dy * gl, dy * a * gd)


def ulp_bf16(ref):
    """Spacing of bf16 at |ref| (fp64 in, fp64 out): 2^(floor(log2 |ref|) - 7), 2^-133 below the smallest normal."""
    _, e = torch.frexp(ref.double().abs())
    e = torch.where(ref == 0, torch.full_like(e, -1000), e)
    return torch.ldexp(torch.ones_like(ref, dtype=F64), (e - 8).clamp(min=-133, max=120))


def act_bound(ref, dtype, A):
    return ulp_bf16(ref) + A if dtype == BF16 else REL_F32 * ref.abs() + A


def act_ratio(got, ref, dtype, A, compare=None):
    """Largest |got - ref| / bound over the elements of `compare` (default: all); inf for a NaN or a wrong infinity."""
    got = got.detach().double().cpu().flatten()
    ref = ref.flatten()
    err = (got - ref).abs()
    over = (ref.abs() >= OUT_MAX[dtype] * (1 - 2.0 ** -10)) & torch.isinf(got) & (torch.sign(got) == torch.sign(ref))
    err = torch.where(over, torch.zeros_like(err), err)
    r = torch.nan_to_num(err / act_bound(ref, dtype, A), nan=float('inf'), posinf=float('inf'))
    if compare is not None:
        r = r[compare.flatten()]
    return r.max().item() if r.numel() else 0.0


def act_excess(emu, ref, dtype):
    """a of the module docstring: the largest |f - ref| - REL |ref| over representable references."""
    rel = REL_BF16 if dtype == BF16 else REL_F32
    ok = torch.isfinite(ref) & torch.isfinite(emu.double()) & (ref.abs() < OUT_MAX[dtype] * (1 - 2.0 ** -10))
    ex = ((emu.double() - ref).abs() - rel * ref.abs()).clamp(min=0)
    return ex[ok].max().item()


def store(t, dtype):
    """The final rounding of a kernel: fp32 registers -> storage type."""
    return t.to(dtype)


# ---- colsum ------------------------------------------------------------------------------------------------------------------------
COLSUM_CASES = ((1, 1, 8), (3, 63, 24), (2, 65, 320), (1, 130, 2048), (2, 257, 2056), (5, 700, 40), (1, 8193, 8))     # B, rows, N
COLSUM_NO_WS = ((3, 63, 24), (2, 257, 2056))
COLSUM_LD_PB_EXTRA, COLSUM_PB_SHIFT = 64, 32


def colsum_nchunks(B, rows):
    """colsum_nchunks of elementwise.hip."""
    want, maxch = (512 + B - 1) // B, (rows + 63) // 64
    return min(max(min(want, maxch), 1), 128)


def colsum_chunks(B, rows):
    """[r0, r1) of every row chunk of a batch; r1 < r0 for a chunk that starts past the last row."""
    nch = colsum_nchunks(B, rows)
    rpc = (rows + nch - 1) // nch
    return [(c * rpc, min(rows, c * rpc + rpc)) for c in range(nch)]


def colsum_ref(g, mutation=None):
    """g [B, rows, N] -> fp64 (per_batch [B, N], total [N])."""
    g = g.double()
    B, rows, N = g.shape
    pb = g.sum(1)
    if mutation == 'chunk_last_row_dropped':
        r0, r1 = colsum_chunks(B, rows)[0]
        pb = pb - g[:, r1 - 1]
    elif mutation == 'row_counted_twice':
        pb = pb + g[:, 0]
    elif mutation == 'columns_past_2048_dropped':
        pb = pb.clone()
        pb[:, 2048:] = 0
    return pb, pb.sum(0)


def sumpool_ref(g, mutation=None):
    """g [B, 2H, 2W, C] -> fp64 [B, H, W, C]."""
    B, H2, W2, C = g.shape
    v = g.double().view(B, H2 // 2, 2, W2 // 2, 2, C)
    out = v.sum((2, 4))
    return out - v[:, :, 1, :, 1] if mutation == 'tap_missing' else out


def zero_insert_ref(g, H, W, mutation=None):
    """g [B, Ho, Wo, C] -> [B, H, W, C] of g's dtype: out[2h][2w] = g[h][w], +0 elsewhere."""
    B, Ho, Wo, C = g.shape
    if mutation == 'odd_as_even':       # rows and columns laid out as if H = 2 Ho, W = 2 Wo
        full = torch.zeros(B, 2 * Ho, 2 * Wo, C, dtype=g.dtype)
        full[:, ::2, ::2] = g
        return full.flatten()[:B * H * W * C].view(B, H, W, C).clone()
    out = torch.zeros(B, H, W, C, dtype=g.dtype)
    out[:, ::2, ::2] = g
    return out


# ---- losses ------------------------------------------------------------------------------------------------------------------------
# S, per-sample shape, alpha, NaNs as (tensor, sample, flat index; -1 = last), sample with x == y_real (w clipped at 1e-5)
LossCase = collections.namedtuple('LossCase', 'S shape alpha nans clip')
LOSS_CASES = (
    LossCase(1, (1, 1, 1), 1.0, (), None),
    LossCase(1, (1, 1, 1), 1.2, (('x', 0, 0),), None),                                       # every sample dropped
    LossCase(1, (1, 1, 4356), 1.2, (), 0),
    LossCase(3, (1, 1, 255), 1.0, (('y_real', 1, 64),), None),
    LossCase(3, (4, 16, 32), 1.2, (('y_fake', 2, 255),), 0),                                 # n = 2048
    LossCase(3, (1, 1, 2049), 1.0, (('x', 0, -1),), None),
    LossCase(3, (1, 1, 2048), 1.0, (('x', 0, 64), ('y_real', 1, 0), ('y_fake', 2, -1)), None),     # every sample dropped
    LossCase(9, (1, 1, 255), 1.2, (('y_fake', 8, -1), ('y_real', 0, 0)), 4),                 # two dropped
    LossCase(9, (1, 1, 1), 1.0, (('x', 3, 0),), None),
    LossCase(9, (4, 33, 33), 1.0, (('y_real', 3, -1),), None),                               # n = 4356
    LossCase(9, (4, 33, 33), 1.2, (('x', 5, 255), ('y_fake', 6, 64)), 1),
    LossCase(9, (1, 1, 2049), 1.0, (), None),
)
LOSS_TOL = 1e-5


def loss_case_id(c):
    n = int(np.prod(c.shape))
    return f'S{c.S}-n{n}-a{c.alpha}-' + ('+'.join(f'{t}{s}@{i}' for t, s, i in c.nans) or 'nonan') + (f'-clip{c.clip}' if c.clip is not None else '')


def loss_inputs(c):
    """fp32 x, y_real, y_fake [S, *shape] (+ s0, s1, w [S] for the v form)."""
    g = torch.Generator().manual_seed(900 + 31 * c.S + int(np.prod(c.shape)) + int(10 * c.alpha) + len(c.nans))
    x, yr, yf = (torch.randn(c.S, *c.shape, generator=g) for _ in range(3))
    if c.clip is not None:
        x[c.clip] = yr[c.clip]
    for name, s, i in c.nans:
        dict(x=x, y_real=yr, y_fake=yf)[name][s].view(-1)[i] = float('nan')
    s0, s1, w = (torch.rand(c.S, generator=g) * 0.9 + 0.1 for _ in range(3))
    return dict(x=x, y_real=yr, y_fake=yf, s0=s0, s1=s1, w=w)


def g_loss_ref64(x, yr, yf, alpha, scale, mutation=None):
    """Generator loss of oracle/sid_ref.generator_loss_ref (scale = loss_scaling_G / batch_gpu_total) in closed form, fp64 ->
    (loss, dx, dyr, dyf, dropped [S])."""
    x, yr, yf = x.double(), yr.double(), yf.double()
    S = x.shape[0]
    nan = lambda t: torch.isnan(t).flatten(1).any(1)  # noqa: E731
    drop = nan(x) if mutation == 'nan_in_x_only' else nan(x) | nan(yr) | nan(yf)
    w = (x - yr).abs().flatten(1).mean(1)
    if mutation != 'w_unclipped':
        w = w.clip(min=1e-5)
    w = w.view(S, *[1] * (x.dim() - 1))
    d, e = yr - yf, yr - x
    al = -alpha if mutation == 'alpha_sign' else alpha
    terms = d * (e - al * d) / w
    dyr, dyf, dx = scale * (e + (1 - 2 * al) * d) / w, scale * (-e + 2 * al * d) / w, scale * (-d) / w
    loss = terms[~drop].sum() * scale
    if mutation != 'dropped_keeps_gradient':
        dx, dyr, dyf = (torch.where(drop.view_as(w), torch.zeros_like(t), t) for t in (dx, dyr, dyf))
    return loss, dx, dyr, dyf, drop


def fake_loss_v_ref64(o, images, noise, s0, s1, w, scale):
    """scale * sum_s w_s |o_s - (s0 noise - s1 images)_s|^2 over samples without a NaN in o or v*; d o."""
    v = s0.double().view(-1, 1, 1, 1) * noise.double() - s1.double().view(-1, 1, 1, 1) * images.double()
    drop = torch.isnan(o).flatten(1).any(1) | torch.isnan(v).flatten(1).any(1)
    d = o.double() - v
    loss = ((d ** 2).sum((1, 2, 3)) * w.double())[~drop].sum() * scale
    grad = 2 * scale * w.double().view(-1, 1, 1, 1) * d
    grad[drop] = 0
    return loss, grad, drop


def loss_ratio(got_loss, ref_loss, grads, ref_grads, drop):
    """Largest miss / bound: value 1e-5 relative, every gradient 1e-5 of its maximum inside each sample; a dropped sample's
    gradient must be exactly 0 (inf otherwise); NaN or inf anywhere -> inf."""
    got_loss, ref_loss = float(got_loss), float(ref_loss)
    if not math.isfinite(got_loss):
        return float('inf')
    worst = abs(got_loss - ref_loss) / (LOSS_TOL * abs(ref_loss)) if ref_loss != 0 else (0.0 if got_loss == 0 else float('inf'))
    for g, r in zip(grads, ref_grads):
        g, r = g.detach().double().cpu().flatten(1), r.detach().double().cpu().flatten(1)
        if not torch.isfinite(g).all():
            return float('inf')
        if drop.any() and float(g[drop].abs().max()) != 0.0:
            return float('inf')
        keep = ~drop
        if keep.any():
            scale = r[keep].abs().amax(1)
            err = (g[keep] - r[keep]).abs().amax(1)
            worst = max(worst, float((err / (LOSS_TOL * scale.clamp(min=1e-300))).max()))
    return worst


# ---- optimizer ---------------------------------------------------------------------------------------------------------------------
AdamCfg = collections.namedtuple('AdamCfg', 'name lr betas eps weight_decay decoupled clip grad_scale')
ADAM_CFGS = (AdamCfg('recipe', 1e-3, (0.0, 0.999), 1e-8, 0.0, False, None, 1.0),
             AdamCfg('everything', 3e-3, (0.9, 0.99), 1e-6, 0.02, False, 0.25, 0.5),
             AdamCfg('adamw', 3e-3, (0.0, 0.999), 1e-8, 0.05, True, None, 1.0))
ADAM_LARGE = 4194304 + 1203          # 4096 blocks x 256 threads x 4 = one pass; the second has 300 vector bodies and a tail of 3
ADAM_N = (1, 3, 4, 5, 1027, ADAM_LARGE)
ADAM_BETAS = (0.0, 0.3, 0.5, 0.999, 0.3)
ADAM_TOL, ADAM_TOL_TORCH = 1e-6, 2e-6
ADAM_KEEP_GRAD_STEP = 1              # the step run with zero_grad=False


def adam_steps(n):
    return 2 if n == ADAM_LARGE else 5


def adam_beta(n, step):
    return (0.3, 0.999)[step] if n == ADAM_LARGE else ADAM_BETAS[step]


def adam_special(n):
    """Indices that get NaN / +inf / -inf: three of the vector body (and three of the second grid-stride pass), and the tail."""
    body = n - n % 4
    idx = list(range(min(3, body)))
    if n > 4194304 + 16:
        idx += [4194304 + 8, 4194304 + 9, 4194304 + 10]
    return idx + list(range(body, n))


def adam_grad(n, step, seed=5):
    """The gradient of a step: randn at scale 10^(step - 2), a few zero / tiny entries (eps matters there), NaN / +-inf rotating
    over adam_special(n)."""
    g = torch.randn(n, generator=torch.Generator().manual_seed(seed * 100 + step)) * 10.0 ** (step - 2)
    if n >= 16:
        g[8:12] = torch.tensor([0.0, 1e-9, 1e-7, -1e-9])
    kinds = (float('nan'), float('inf'), -float('inf'))
    for j, i in enumerate(adam_special(n)):
        g[i] = kinds[(j + step) % 3]
    return g


def adam_ema_ref(p, g, ema, st, cfg, beta, mutation=None):
    """One step of oracle/sid_ref.adam_step_ref + ema_update_ref in the tensors' own precision, in place (st: step, m, v)."""
    g = torch.nan_to_num(g * cfg.grad_scale, nan=0.0, posinf=1e5, neginf=-1e5)
    if cfg.clip is not None:
        g = g.clamp(-cfg.clip, cfg.clip)
    st['step'] = st.get('step', 0) + 1
    b1, b2 = cfg.betas
    decoupled = cfg.decoupled != (mutation == 'decay_swapped')
    if cfg.weight_decay != 0:
        if decoupled:
            p.mul_(1 - cfg.lr * cfg.weight_decay)
        else:
            g = g + cfg.weight_decay * p
    m = st.setdefault('m', torch.zeros_like(p))
    v = st.setdefault('v', torch.zeros_like(p))
    m.lerp_(g, 1 - b1)
    v.mul_(b2).addcmul_(g, g, value=1 - b2)
    bc1, bc2 = 1 - b1 ** st['step'], 1 - b2 ** st['step']
    if mutation == 'eps_inside_root':
        denom = (v / bc2 + cfg.eps).sqrt()
    else:
        denom = (v.sqrt() / (bc2 if mutation == 'bc2_for_sqrt' else math.sqrt(bc2))).add_(cfg.eps)
    p.addcdiv_(m, denom, value=-cfg.lr / bc1)
    ema.copy_(ema.lerp(p, beta) if mutation == 'ema_reversed' else p.lerp(ema, beta))


def max_rel(got, ref, idx=None):
    """close() of tests/test_gpu_ops.py as a number: max|got - ref| / max|ref| (over idx), inf for a non-finite result."""
    got, ref = got.detach().double().cpu().flatten(), ref.detach().double().cpu().flatten()
    if idx is not None:
        got, ref = got[idx], ref[idx]
    if got.numel() == 0:
        return 0.0
    if not torch.isfinite(got).all():
        return float('inf')
    return (got - ref).abs().max().item() / (ref.abs().max().item() + 1e-12)


def adam_ratio(got, ref, n, tol=ADAM_TOL):
    """The larger of max_rel over the ordinary and over the NaN / inf elements, in units of the bound."""
    sp = torch.zeros(n, dtype=torch.bool)
    sp[adam_special(n)] = True
    return max(max_rel(got, ref, ~sp), max_rel(got, ref, sp)) / tol


# ---- weight preparation ------------------------------------------------------------------------------------------------------------
CAST_N = (1, 7, 8, 9, 2047, 2049)
CAST_LOW = (0, 1, 0x7fff, 0x8000, 0x8001, 0xffff)
SCALE_CAST_TABLES = ((4100,), (1, 2049), (7, 8, 2047, 2048, 4100))
TRANSPOSE_CASES = ((8, 8, 1), (72, 136, 9), (64, 64, 1), (320, 40, 9), (8, 200, 1))          # N, K, T
TRANSPOSE_F32_ONLY = ((4, 320, 9), (320, 4, 9))
TRANSPOSE_TABLES = tuple((c,) for c in TRANSPOSE_CASES) + (((72, 136, 9), (8, 200, 1)), TRANSPOSE_CASES)
TRANSPOSE_TABLES_F32 = TRANSPOSE_TABLES + tuple((c,) for c in TRANSPOSE_F32_ONLY) + (TRANSPOSE_F32_ONLY,)


def cast_words():
    """(h << 16) | low for every bf16 pattern h and low of CAST_LOW, as fp32 [65536 * 6]."""
    h = torch.arange(65536, dtype=torch.int64).view(-1, 1) << 16
    w = (h | torch.tensor(CAST_LOW, dtype=torch.int64).view(1, -1)).flatten()
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32).view(F32)


def cast_ref(x, mutation=None):
    if mutation == 'truncation':
        return (x.contiguous().view(torch.int32) >> 16).to(torch.int16).view(BF16)
    return x.to(BF16)


def cast_equal(got, ref):
    """Bit-equal, except that any NaN equals any NaN."""
    got, ref = got.cpu(), ref.cpu()
    gn, rn = torch.isnan(got), torch.isnan(ref)
    return bool(torch.equal(gn, rn)) and bits_equal(torch.where(gn, torch.zeros_like(got), got), torch.where(rn, torch.zeros_like(ref), ref))


def finite_bf16(n, seed):
    """n random finite bf16 values (as bf16)."""
    g = torch.Generator().manual_seed(seed)
    p = torch.randint(0, 0x7f80, (n,), generator=g, dtype=torch.int32) | (torch.randint(0, 2, (n,), generator=g, dtype=torch.int32) << 15)
    return torch.where(p >= 2 ** 15, p - 2 ** 16, p).to(torch.int16).view(BF16)


def transpose_ref(src, N, K, T, mutation=None):
    """src [N][T][K] -> [K][T reversed][N]."""
    out = src.view(N, T, K).permute(2, 1, 0)
    return (out if mutation == 'taps_not_reversed' else out.flip(1)).contiguous()


def tw_table(jobs, tile):
    """Job table of sidlsg_transpose_w*_batched as HipUNet2DCondition._build_transpose_plan writes it.  jobs: (src ptr, dst ptr, N,
    K, T); tile: 32 (fp32 sources) or 64 (bf16 sources) -> (uint8 CPU tensor, njobs, nblocks)."""
    rec = np.zeros(len(jobs), dtype=np.dtype([('src', '<u8'), ('dst', '<u8'), ('N', '<i4'), ('K', '<i4'), ('T', '<i4'), ('blk0', '<i4')]))
    blk = 0
    for i, (src, dst, n, k, t) in enumerate(jobs):
        rec[i] = (src, dst, n, k, t, blk)
        blk += t * ((n + tile - 1) // tile) * ((k + tile - 1) // tile)
    return torch.from_numpy(rec.view(np.uint8).copy()), len(jobs), blk


def sc_table(jobs):
    """Job table of sidlsg_scale_cast_ranges as _build_prescale_plan writes it.  jobs: (src ptr, dst ptr, n, scale)."""
    rec = np.zeros(len(jobs), dtype=np.dtype([('src', '<u8'), ('dst', '<u8'), ('n', '<i4'), ('blk0', '<i4'), ('scale', '<f4'), ('pad', '<i4')]))
    blk = 0
    for i, (src, dst, n, scale) in enumerate(jobs):
        rec[i] = (src, dst, n, blk, scale, 0)
        blk += (n + 2047) // 2048
    return torch.from_numpy(rec.view(np.uint8).copy()), len(jobs), blk


# ---- timestep embedding ------------------------------------------------------------------------------------------------------------
TEMB_T, TEMB_DIMS = (0, 1, 999), (8, 320, 1280)
TEMB_TOL = {BF16: 1.2e-2, F32: 2e-4}             # tests/test_gpu_ops.py::test_small_ops, tests/test_gpu_fp32.py::test_small_ops_f32


def timestep_ref64(t, dim):
    half = dim // 2
    ang = t.double()[:, None] * torch.exp(-math.log(10000.0) * torch.arange(half, dtype=F64) / half)[None]
    return torch.cat([ang.cos(), ang.sin()], 1)


MUTATIONS = {
    'activations': ('tanh_gelu', 'sigmoid_gelu', 'silu_grad_no_x'),
    'colsum': ('chunk_last_row_dropped', 'row_counted_twice', 'columns_past_2048_dropped'),
    'sumpool2x2': ('tap_missing',),
    'zero_insert2': ('odd_as_even',),
    'g_loss': ('nan_in_x_only', 'w_unclipped', 'alpha_sign', 'dropped_keeps_gradient'),
    'adam': ('bc2_for_sqrt', 'eps_inside_root', 'decay_swapped', 'ema_reversed'),
    'cast': ('truncation',),
    'transpose': ('taps_not_reversed',),
}


# ---- the measurement behind A ------------------------------------------------------------------------------------------------------
def measure_tolerance(path=None):
    """a and A per (dtype, op, variant) -> {(dtype, op, variant): a}; writes the table."""
    out = {}
    lines = ['The kernels\' activation formulas (tests/elementwise_cases.py act_emulated: common.h in fp32 on the CPU, before the final rounding)',
             'against the fp64 reference over the sweep of every bf16 bit pattern (fp32: + 65,536 random finite fp32 patterns).',
             'a = max(|f - ref| - REL |ref|, 0), REL = 2^-16 (bf16 kernels) / 2e-5 (fp32 kernels); A = max(2 a, 1e-6).', '',
             'kernels  op         inputs      a            A = max(2a, 1e-6)   constant in the module']
    for dtype, nm in ((BF16, 'bf16'), (F32, 'fp32')):
        for op in ACT_OPS:
            for variant in ACT_VARIANTS:
                i = sweep_inputs(op, variant, dtype)
                ref = act_ref64(op, i['x'], i['a'], i['dy'])
                emu = act_emulated(op, i['x'], i['a'], i['dy'], dtype)
                fin = torch.isfinite(i['x'].double())
                a = max(act_excess(e[fin], r[fin], dtype) for e, r in zip(emu, ref))
                out[(dtype, op, variant)] = a
                lines.append(f'{nm:7s}  {op:9s}  {variant:6s}  {a:11.3e}  {max(2 * a, A_FLOOR):11.3e}         {A_OF[dtype]:.2e}')
    lines += ['', 'tests/test_gpu_elementwise_edges.py on an MI355X, largest |got - ref| / bound per kernel:']
    lines += [f'  {k:28s} {v:.3f}' for k, v in MEASURED_MI355X.items()]
    text = '\n'.join(lines) + '\n'
    if path:
        with open(path, 'w') as f:
            f.write(text)
    print(text)
    return out


if __name__ == '__main__':
    measure_tolerance(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'elementwise_tolerance.txt'))
