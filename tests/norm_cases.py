"""Shared by tests/test_norm_cases_host.py, tests/test_gpu_ops.py, tests/test_gpu_fp32.py and tests/test_gpu_norm_fp8.py (not a test module): GroupNorm /
LayerNorm inputs whose (sample, group) blocks -- rows for LayerNorm -- all have DIFFERENT statistics, their fp64 reference, the
per-block error metric and three deliberately wrong references.

Why: with iid input of one global mean and scale every (sample, group) has the same mean and rstd to within 1 / sqrt(n) and both
group sums of the backward, mean(dy * gamma) and mean(dy * gamma * xhat), vanish to within 1 / sqrt(n).  A kernel that reads the
statistics of the wrong group or sample, or loses a projection term, then passes.  Here every block has its own scale
sigma = 2^k (k in -2 .. 2), its own mean offset * sigma (offset drawn from a list that reaches 30 or 100 standard deviations), and
dy = a + b * z + noise with per-block a, b ~ N(0, 1), which makes both projection terms O(1).

dx scales with 1 / sigma, so a global max|err| / max|ref| would only see the small-sigma blocks: y and dx are judged per block
(group_rel_err), dgamma / dbeta keep the global metric.
"""
import functools

import torch
import torch.nn.functional as F

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64

# ---- the cases of the GPU tests (tests/test_norm_cases_host.py checks every one of them on the CPU) -------------------------------
OFFSETS_BF16 = (0, 3, -3, 30, -30)
TOL_BF16 = dict(y=1.2e-2, dx=1.5e-2, dgamma=3e-3, dbeta=3e-3)          # the tolerances of test_groupnorm / test_layernorm
# (B, HW, C, G, silu, eps, fork)
GN_CASES_BF16 = (
    # one-pass kernels (gn_small_*): 2 / 1 / 4 groups per block, a ragged pixel count
    (3, 64, 32, 8, 1, 1e-5, True), (2, 64, 1280, 32, 1, 1e-5, False), (3, 256, 320, 32, 0, 1e-5, False), (2, 100, 80, 8, 0, 1e-5, False),
    # forward one-pass, backward two-kernel
    (3, 1024, 320, 32, 1, 1e-5, False),
    # two-kernel path; the per-group kernels (gn_group_*) where they are switched on
    (2, 4096, 320, 32, 0, 1e-5, True), (2, 4096, 640, 32, 1, 1e-5, False), (1, 1100, 320, 32, 1, 1e-5, False), (2, 1024, 1920, 32, 1, 1e-5, False),
    # VAE-like: 4 and 16 channels per group, eps 1e-6
    (1, 16384, 128, 32, 1, 1e-6, False), (1, 4096, 512, 32, 0, 1e-6, False),
)
# deterministic mode with trainable gamma / beta: the two-kernel backward at shapes that otherwise take the one-pass kernels
GN_CASES_DET = ((2, 64, 1280, 32, 1, 1e-5, False), (3, 256, 320, 32, 0, 1e-5, False))
LN_CASES_BF16 = ((100, 320), (257, 1280), (300, 80), (4096, 640))

# fp32 mode: (name, offsets, factor on the tolerances of tests/test_gpu_fp32.py).  A statistics error relative to |mean| grows
# linearly with the offset: 100 / 30 rounds up to 4
TOL_F32 = dict(y=2e-5, dx=5e-5, dgamma=5e-5, dbeta=5e-5)
OFFSET_SETS_F32 = (('off30', (0, 3, -10, 30, -30), 1.0), ('off100', (0, 3, -30, 100, -100), 4.0))
GN_CASES_F32 = ((3, 64, 32, 8, 1, 1e-5, False), (3, 1024, 320, 32, 1, 1e-5, False), (2, 4096, 320, 32, 0, 1e-5, False), (1, 1100, 320, 32, 1, 1e-5, False))
LN_CASES_F32 = ((100, 320), (257, 1280))


# e4m3-output forwards (sidlsg_groupnorm_fwd_fp8 / sidlsg_layernorm_fwd_fp8): the small cases above, judged byte for byte (tests/fp8_cases.py
# byte_oracle).  An element is decidable when the fp64 reference lies further than d = TOL_F32['y'] * (block max |y|) from every midpoint between
# neighbouring e4m3 values -- the project's own fp32 bar for the same per-block metric: the kernels compute y in fp32 from the given bf16 x, and an
# fp32 y within that bar of the reference rounds to the reference's byte.  At most F8_UNDECIDABLE_CAP of a case's elements may be undecidable.
_F8_GN = ((3, 64, 32, 8, 1), (2, 64, 1280, 32, 1), (2, 100, 80, 8, 0), (3, 1024, 320, 32, 1), (2, 4096, 320, 32, 0), (1, 1100, 320, 32, 1))
GN_CASES_F8 = tuple(c for c in GN_CASES_BF16 if c[:5] in _F8_GN)
LN_CASES_F8 = ((100, 320), (257, 1280), (300, 80))
F8_UNDECIDABLE_CAP = 0.05
# gamma * F8_SAT_GAIN on one GroupNorm and one LayerNorm case: |y| passes 448 where |xhat gamma| > 7 -- the few outputs where a 3-sigma input
# meets one of the largest gammas, on either side; they must be the +-448 bytes.  F8_SAT_COUNTS: how many reference outputs round to the +448 /
# -448 byte in each saturating case (the host test asserts these numbers on the reference, the GPU test counts the kernel's bytes against them)
F8_SAT_GAIN = 64.0
GN_CASE_F8_SAT, LN_CASE_F8_SAT = (2, 4096, 320, 32, 0, 1e-5, True), (257, 1280)
F8_SAT_COUNTS = {'gn': (75, 81), 'ln': (6, 15)}
# ids of the cases that also run with one NaN input element
F8_NAN_IDS = ('gn-2-100-80-8-0', 'gn-3-1024-320-32-1', 'ln-300-80', 'ln-257-1280')
# The statistics an e4m3 forward writes are fp32 (mean, rstd), judged against fp64 on the bf16 x: the mean's error in sigma, rstd's relatively.
# The bar is what fp32 arithmetic on these inputs can cost, not what the bf16 outputs tolerate: a variance formed as E[x^2] - mean^2 from a block
# whose mean is `off` standard deviations away works on numbers of size (1 + off^2) sigma^2, every rounding of which is 2^-24 of that relative to
# sigma^2; rstd moves by half of the variance's relative error.  Four such roundings (sum of squares, its division, mean^2, the subtraction) at
# the largest offset of OFFSETS_BF16 give 1.07e-4 -- twenty times below a biased / unbiased slip at n = 256 (2e-3).
F8_STATS_TOL = 4 * 2.0 ** -24 * (1 + max(abs(o) for o in OFFSETS_BF16) ** 2) / 2


def block_stats(x, G, eps):
    """-> (mean, rstd) fp64 [B, G] of x [B, HW, C] (LayerNorm: x.view(rows, 1, C), G = 1)."""
    B, HW, C = x.shape
    xg = x.double().view(B, HW, G, C // G)
    return xg.mean(dim=(1, 3)), torch.rsqrt(xg.var(dim=(1, 3), unbiased=False) + eps)


def f8_sat_bounds(y, d):
    """-> ((lo+, lo-), (hi+, hi-)): how many +448 / -448 bytes a forward within d of the reference y may write -- at least the decidable elements
    whose nearest-even byte is the saturated one, at most those plus the undecidable ones with it as a neighbour."""
    import fp8_cases as fc
    want = fc.ref_bytes(y.double().clamp(-fc.E4M3_MAX, fc.E4M3_MAX).float())
    dec = fc.decidable(y, d)
    lo, hi = fc.neighbours(y)
    out = []
    for byte in (0x7E, 0xFE):
        sure = int((dec & (want == byte)).sum())
        out.append((sure, sure + int((~dec & ((want == byte) | (lo == byte) | (hi == byte))).sum())))
    return tuple(o[0] for o in out), tuple(o[1] for o in out)


def block_d(y, G):
    """d of the decidable-byte oracle: TOL_F32['y'] * (block max |y|), broadcast to y's shape [B, HW, C]."""
    B, HW, C = y.shape
    blk = y.double().abs().view(B, HW, G, C // G).amax(dim=(1, 3), keepdim=True)
    return (TOL_F32['y'] * blk).expand(B, HW, G, C // G).reshape(B, HW, C)


def f8_cases():
    """-> [(id, kind, case, gain)] of every e4m3-output forward case: kind 'gn' / 'ln'; gain multiplies gamma (the saturating cases)."""
    out = [('gn-' + gn_id(c), 'gn', c, 1.0) for c in GN_CASES_F8] + [(f'ln-{c[0]}-{c[1]}', 'ln', c, 1.0) for c in LN_CASES_F8]
    return out + [('gn-' + gn_id(GN_CASE_F8_SAT) + '-sat', 'gn', GN_CASE_F8_SAT, F8_SAT_GAIN), (f'ln-{LN_CASE_F8_SAT[0]}-{LN_CASE_F8_SAT[1]}-sat', 'ln', LN_CASE_F8_SAT, F8_SAT_GAIN)]


@functools.lru_cache(maxsize=None)
def f8_case(kind, case, gain):
    """dict(x bf16 [B, HW, C], gam, bet, G, eps, silu, y fp64 [B, HW, C], mean, rstd): callers must not modify the tensors."""
    if kind == 'gn':
        B, HW, C, G, silu, eps, _ = case
        x, _ = structured_gn(B, HW, C, G, case_seed(case), OFFSETS_BF16, BF16)
    else:
        (B, C), HW, G, silu, eps = case, 1, 1, 0, 1e-5
        x = structured_ln(B, C, case_seed((B, C, 0, 0, 0)), OFFSETS_BF16, BF16)[0].view(B, 1, C)
    gam, bet = affine(C)
    gam = gam * gain
    y = norm_by_formula(x, torch.zeros_like(x), gam, bet, G, eps, silu)['y']
    mean, rstd = block_stats(x, G, eps)
    return dict(x=x, gam=gam, bet=bet, G=G, eps=eps, silu=silu, y=y, mean=mean, rstd=rstd)


def gn_id(case):
    return '-'.join(str(v) for v in case[:5]) + ('-fork' if case[6] else '')


def case_seed(case):
    """One seed per case: a fixed function of its numbers (never of anything measured)."""
    return 1000 + sum(int(v * (i + 1)) for i, v in enumerate(case[:5]))


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def _structure(B, HW, C, G, seed, offsets):
    g = torch.Generator().manual_seed(seed)
    nb = B * G
    z = torch.randn(B, HW, G, C // G, generator=g, dtype=F64)
    sigma = torch.pow(2.0, torch.randint(-2, 3, (nb,), generator=g).double()).view(B, 1, G, 1)
    # every offset of the list is used (where there are at least as many blocks as offsets): a random permutation of a round robin
    off = torch.tensor(offsets, dtype=F64)[torch.randperm(nb, generator=g) % len(offsets)].view(B, 1, G, 1)
    a, b = (torch.randn(nb, generator=g, dtype=F64).view(B, 1, G, 1) for _ in range(2))
    noise, knoise = (torch.randn(B, HW, G, C // G, generator=g, dtype=F64) for _ in range(2))
    x = z * sigma + off * sigma
    dy = a + b * z + 0.5 * noise
    dk = 0.5 * knoise / sigma          # a residual-branch gradient of dx's own scale (dx ~ 1 / sigma)
    return tuple(t.reshape(B, HW, C) for t in (x, dy, dk))


def structured_gn(B, HW, C, G, seed, offsets, dtype):
    """-> (x, dy) of shape [B, HW, C] in `dtype`: see the module docstring."""
    x, dy, _ = _structure(B, HW, C, G, seed, offsets)
    return x.to(dtype), dy.to(dtype)


def structured_gn_residual(B, HW, C, G, seed, offsets, dtype):
    """The gradient that reaches x through its other consumer in the fork=True cases (same generator stream as structured_gn)."""
    return _structure(B, HW, C, G, seed, offsets)[2].to(dtype)


def structured_ln(rows, C, seed, offsets, dtype):
    """-> (x, dy) of shape [rows, C]: one (sigma, mu, a, b) per row."""
    x, dy, _ = _structure(rows, 1, C, 1, seed, offsets)
    return x.view(rows, C).to(dtype), dy.view(rows, C).to(dtype)


def affine(C):
    """gamma, beta (fp32) as in test_groupnorm / test_layernorm."""
    gam = torch.randn(C, generator=torch.Generator().manual_seed(2)) * 0.5 + 1
    bet = torch.randn(C, generator=torch.Generator().manual_seed(3)) * 0.3
    return gam, bet


# ---- references --------------------------------------------------------------------------------------------------------------------
def gn_reference(x, dy, gam, bet, G, eps, silu, dk=None, dtype=F64):
    """F.group_norm (+ F.silu) under autograd in `dtype` on [B, HW, C] inputs -> dict(y, dx, dgamma, dbeta) in `dtype`."""
    xr, gr, br = (t.to(dtype).requires_grad_() for t in (x, gam, bet))
    y = F.group_norm(xr.permute(0, 2, 1), G, gr, br, eps).permute(0, 2, 1)
    if silu:
        y = F.silu(y)
    loss = (y * dy.to(dtype)).sum()
    if dk is not None:
        loss = loss + (xr * dk.to(dtype)).sum()
    loss.backward()
    return dict(y=y.detach(), dx=xr.grad, dgamma=gr.grad, dbeta=br.grad)


def ln_reference(x, dy, gam, bet, eps, dtype=F64):
    xr, gr, br = (t.to(dtype).requires_grad_() for t in (x, gam, bet))
    y = F.layer_norm(xr, (x.shape[-1],), gr, br, eps)
    y.backward(dy.to(dtype))
    return dict(y=y.detach(), dx=xr.grad, dgamma=gr.grad, dbeta=br.grad)


def norm_by_formula(x, dy, gam, bet, G, eps, silu, mutation=None):
    """The same operation written out in fp64 from explicit per-(sample, group) statistics, so that it can be made wrong on purpose:
      mutation None            -- equals gn_reference (the host test asserts that)
               'next_group'    -- every group uses (mean, rstd) of group g + 1
               'next_sample'   -- every sample uses (mean, rstd) of sample b + 1
               'no_projection' -- dx = rstd * d * gamma: both projection terms dropped
    LayerNorm is the case G = 1 with the rows as samples ([rows, 1, C])."""
    B, HW, C = x.shape
    xg = x.double().view(B, HW, G, C // G)
    mean = xg.mean(dim=(1, 3), keepdim=True)
    rstd = torch.rsqrt(xg.var(dim=(1, 3), unbiased=False, keepdim=True) + eps)
    if mutation == 'next_group':
        mean, rstd = mean.roll(-1, 2), rstd.roll(-1, 2)
    elif mutation == 'next_sample':
        mean, rstd = mean.roll(-1, 0), rstd.roll(-1, 0)
    ga, be = gam.double().view(1, 1, G, C // G), bet.double().view(1, 1, G, C // G)
    xh = (xg - mean) * rstd
    u = xh * ga + be
    d = dy.double().view(B, HW, G, C // G)
    y = u
    if silu:
        s = torch.sigmoid(u)
        y = u * s
        d = d * (s * (1 + u * (1 - s)))
    dg = d * ga
    dx = rstd * dg
    if mutation != 'no_projection':
        dx = rstd * (dg - dg.mean(dim=(1, 3), keepdim=True) - xh * (dg * xh).mean(dim=(1, 3), keepdim=True))
    return dict(y=y.reshape(B, HW, C), dx=dx.reshape(B, HW, C), dgamma=(d * xh).sum(dim=(0, 1)).reshape(C), dbeta=d.sum(dim=(0, 1)).reshape(C))


# ---- metrics -----------------------------------------------------------------------------------------------------------------------
def group_rel_err(got, ref, G):
    """max over the (sample, group) blocks of max|got - ref| / max|ref| inside the block; [B, HW, C] tensors.  A non-finite `got`
    gives inf."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, f'shape {tuple(got.shape)} vs {tuple(ref.shape)}'
    if not torch.isfinite(got).all():
        return float('inf')
    B, HW, C = ref.shape
    err = (got - ref).abs().view(B, HW, G, C // G).amax(dim=(1, 3))
    scale = ref.abs().view(B, HW, G, C // G).amax(dim=(1, 3)) + 1e-30
    return (err / scale).max().item()


def row_rel_err(got, ref):
    """group_rel_err for LayerNorm: one block per row of [rows, C]."""
    return group_rel_err(got.reshape(got.shape[0], 1, -1), ref.reshape(ref.shape[0], 1, -1), 1)


def global_rel_err(got, ref):
    """max|got - ref| / max|ref| over the whole tensor (dgamma / dbeta: the metric of the existing tests)."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, f'shape {tuple(got.shape)} vs {tuple(ref.shape)}'
    if not torch.isfinite(got).all():
        return float('inf')
    return ((got - ref).abs().max() / (ref.abs().max() + 1e-30)).item()


# ---- a case's inputs and fp64 reference, computed once per process for the cases that more than one test uses ------------------------
def _gn_case(case, offsets, dtype):
    B, HW, C, G, silu, eps, fork = case
    seed = case_seed(case)
    x, dy = structured_gn(B, HW, C, G, seed, offsets, dtype)
    dk = structured_gn_residual(B, HW, C, G, seed, offsets, dtype) if fork else None
    gam, bet = affine(C)
    return dict(x=x, dy=dy, dk=dk, gam=gam, bet=bet, ref=gn_reference(x, dy, gam, bet, G, eps, silu, dk))


_gn_case_cached = functools.lru_cache(maxsize=None)(_gn_case)


def gn_case(case, offsets, dtype):
    """dict(x, dy, dk, gam, bet, ref): callers must not modify the tensors (small cases are shared between tests)."""
    B, HW, C = case[:3]
    return (_gn_case_cached if B * HW * C <= (1 << 20) else _gn_case)(case, tuple(offsets), dtype)


def ln_case(case, offsets, dtype):
    rows, C = case
    x, dy = structured_ln(rows, C, case_seed((rows, C, 0, 0, 0)), offsets, dtype)
    gam, bet = affine(C)
    return dict(x=x, dy=dy, gam=gam, bet=bet, ref=ln_reference(x, dy, gam, bet, 1e-5))
