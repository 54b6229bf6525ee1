"""Shared by tests/test_attn_cases_host.py and tests/test_gpu_attn_widths.py (not a test module): the case tables of the attention
tests, inputs whose keys can be told apart, their fp64 reference, a CPU emulation of the rounding the kernels are allowed, and the
per-(batch, head) error metric.

Why: with iid randn inputs every key of a row weighs about 1 / Nk, and close() of tests/test_gpu_ops.py measures against max|ref| of
the whole tensor.  A key that is dropped, counted twice or wrongly masked then costs 1 / Nk of the output and passes.

Needle inputs.  q, k, v, dO are bf16 randn.  Every (batch, head) pair has ONE needle key j: K[j] = a u_h, V[j] *= 4, and every query
gets + a u_h (u_h a unit vector per head with u_h[0] = 0, a^2 = NEEDLE_NATS sqrt(D)) in place of its own component along u_h: the
needle's score is 5.5 nats for every query, the others' are N(0, 1 + 5.5 D^-1/2), and its softmax share is neither ~0 nor ~1
(test_attn_cases_host.py asserts 0.005 <= share <= 0.97 for every query; measured 0.0095 .. 0.81, and 0.06 .. 0.88 below 61 keys.
With the queries' own component along u_h left in, the needle's score spreads by sqrt(5.5) D^-1/4 nats and single queries of the
D = 8 cases left that range on both sides).  Losing, doubling or misplacing it is an O(1) error in O, dQ, dK[j] and dV[j].  The positions rotate over the pairs of a launch
(needle_positions): pair 0 always has the last key Nk - 1, the others walk through 0, 15, 16, 31, 32, 63, 64, Nk - 2, Nk // 2 and a
key in the second 64 of a 128-key block (the second key tile of a wave of attn_dkdv_kernel<48, 2>); the walk starts at another place
for the other member of a DP pair, for the `_ps` twin and for the other length, so the launches of one width cover the list.
Below 61 keys the boost is 1 + ln Nk nats: 5.5 nats among 13 keys would be a share of ~1, and counting such a needle twice changes little.
With ONE query (the (1, 77) shape) it is 3.5 nats: a slice's dQ and dK are then one row times one number, P (dP - delta), nothing
averages over queries, and the error of delta (taken from the bf16-rounded O, which the needle's 4 v dominates) alone reached 0.048
(dQ) and 0.108 (dK) of the slice maximum in the emulation at 5.5 nats -- above the 5e-2 a bound may have, so `a` is weakened, not the
bound: 0.015 / 0.014 at 3.5 nats.

Biased inputs (forward only).  The needle input with column 0 of every head set to + beta in q and - beta in k, beta^2 D^-1/2 = 12:
every real score moves down by 12 nats, the softmax is unchanged, and a phantom key (a zero row read past Nk that escaped the mask)
would weigh e^12 real ones.  Not for gradients: dQ[:, 0] is then beta times a cancellation (sum dS = 0) and the bf16 rounding of dS
alone misses 2e-2 there; in the backward a phantom row meets zero operands anyway.

attn_ref64: fp64 softmax attention, gradients by torch autograd; `mutation` makes it wrong on purpose (the host test proves that every
such reference misses the bounds by more than 10x).  attn_emulated: the kernels' ALGORITHM on the CPU in fp32 -- 64-key tiles, a
running maximum that only moves when a tile exceeds it by 2^8 (so exponentials reach 2^8), P and dS rounded to bf16 in front of the
second contraction, the ones-column denominator (a sum of ROUNDED probabilities) where D == DP - 8, delta from the rounded O, outputs
rounded to bf16.  It models the rounding this project tolerates; it is not the code under test.

Bounds (close_slices: max|err| <= tol * max|ref| inside every (batch, head) slice):
  * forward FWD_TOL = 1.2e-2, the bf16 bound of tests/test_gpu_ops.py (the emulation measures 0.0065 at most);
  * LSE: LSE_TOL_BITS = 2e-2 absolute in the log2 domain (2^-8 relative error of l is 5.6e-3 bits; emulation 3.7e-3 at most, on the ones-column forward);
  * gradients GRAD_TOL: twice the emulation's largest per-slice error over every gradient case of this file, floor 2e-2, at most
    5e-2 (the kernels add in another order than the emulation).  Measured by `python tests/attn_cases.py`, which writes
    profiles/attn_needle_tolerance.txt:
        dq 0.0149 -> 3.0e-2        dk 0.0139 -> 2.8e-2        dv 0.0106 -> 2.2e-2
  * fp32 kernels: the bounds of tests/test_gpu_fp32.py (2e-5 forward, 5e-5 gradients), per slice.
Measured on the MI355X (tests/test_gpu_attn_widths.py, largest per-slice figure of the whole file; MEASURED_MI355X below):
o 0.0065, biased o 0.0066, LSE 0.0038 bits, dq 0.0149, dk 0.0139, dv 0.0106, causal o 0.0039; the fp32 causal kernel 1.2e-6, the fp32 attention below 5e-6 (printed as 0.00000).
"""
import collections
import functools
import math
import os

import torch
import torch.nn.functional as F

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
LOG2E = 1.4426950408889634
NEEDLE_NATS = 5.5            # a^2 D^-1/2
LONE_QUERY_NATS = 3.5        # Nq = 1 (module docstring)
BIAS_NATS = 12.0             # beta^2 D^-1/2
SHARE_RANGE = (0.005, 0.97)

FWD_TOL = 1.2e-2
WHOLE_GRAD_TOL = 2e-2        # close() of tests/test_gpu_ops.py over the whole tensor: kept as a second assertion
LSE_TOL_BITS = 2e-2
GRAD_TOL = dict(dq=3.0e-2, dk=2.8e-2, dv=2.2e-2)
GRAD_TOL_FLOOR, GRAD_TOL_CEILING = 2e-2, 5e-2
F32_TOL = dict(o=2e-5, dq=5e-5, dk=5e-5, dv=5e-5)

# largest figures of tests/test_gpu_attn_widths.py on an MI355X (pytest -s prints them), each with the case that gave it
MEASURED_MI355X = {
    'o': (0.00651, 'self-d128-n200-b2h4'), 'biased o': (0.00657, 'self-d48-n127-b2h4-ps'), 'lse bits': (0.00382, 'cross-d40-q130k77-b2h4-ps'),
    'dq': (0.01485, 'cross-d8-q1k77-b2h4'), 'dk': (0.01390, 'self-d160-n63-b2h4'), 'dv': (0.01057, 'cross-d8-q130k63-b2h4'),
    'causal o': (0.00392, 'self-d48-n17-b2h2'),
}

ADMITTED_DP = (16, 32, 48, 64, 80, 96, 128, 160)        # the head widths attention.hip is tiled for
WIDTHS = tuple(d for d in range(8, 161, 8) if (d + 15) // 16 * 16 in ADMITTED_DP)
REFUSED_WIDTHS = (104, 112, 136, 144, 0, 4, 168)

# kind 'self': q | k | v packed in one [B, N, 3C] buffer (ops.self_attention); 'cross': q [B, Nq, C], k | v [B, Nk, 2C]
Case = collections.namedtuple('Case', 'kind B H Nq Nk D ps')


def case_id(c):
    n = f'n{c.Nq}' if c.kind == 'self' else f'q{c.Nq}k{c.Nk}'
    return f'{c.kind}-d{c.D}-{n}-b{c.B}h{c.H}' + ('-ps' if c.ps else '')


def _both(kind, B, H, Nq, Nk, D):
    return [Case(kind, B, H, Nq, Nk, D, ps) for ps in (False, True)]


# every admitted width, N = 200 (3 whole key tiles + a ragged one, a ragged second query block) and N = 128 (whole tiles: the
# instantiations without masking, the rotated walk of the backward)
SWEEP_CASES = tuple(c for D in WIDTHS for N in (200, 128) for c in _both('self', 2, 4, N, N, D))
EDGE_D = (8, 40, 48, 96, 128, 160)
SELF_EDGE_N = (1, 15, 16, 17, 63, 64, 65, 127, 129)
CROSS_EDGE = ((130, 1), (130, 13), (130, 63), (130, 64), (130, 65), (130, 77), (129, 128), (1, 77))
EDGE_CASES = tuple(c for D in EDGE_D for N in SELF_EDGE_N for c in _both('self', 2, 4, N, N, D)) + \
    tuple(c for D in EDGE_D for nq, nk in CROSS_EDGE for c in _both('cross', 2, 4, nq, nk, D))
# attn_dkdv_kernel<48, 2> (Nk >= 1024): a ragged last 128-key block, a needle in the second half of a block
LONG_CASES = tuple(c for D in (40, 48) for c in _both('cross', 2, 4, 129, 1032, D) + _both('self', 2, 2, 1032, 1032, D))
DQ_ONLY_CASES = tuple(c for D in (96, 128) for c in _both('cross', 2, 4, 130, 77, D))       # dK = dV = NULL
FUSED_CASES = tuple(c for B, H, N in ((1, 2, 512), (2, 2, 1024)) for c in _both('self', B, H, N, N, 48))
GRAD_CASES = SWEEP_CASES + EDGE_CASES + LONG_CASES + DQ_ONLY_CASES + FUSED_CASES
BIASED_CASES = EDGE_CASES + LONG_CASES                      # forward + LSE only
F32_WIDTHS = (4, 12, 24, 48, 56, 88, 96, 120, 128, 152)
F32_CASES = tuple(Case('self', 2, 4, 200, 200, D, False) for D in F32_WIDTHS)
CAUSAL_WIDTHS = tuple(range(8, 129, 8))
CAUSAL_CASES = tuple(Case('self', 2, 2, N, N, D, False) for D in CAUSAL_WIDTHS for N in (17, 77))


def is_ones(D):
    """The forward that takes the softmax denominator from a ones column of V: D == DP - 8."""
    return D % 16 == 8


def case_seed(c):
    """One seed per case: a fixed function of its numbers (never of anything measured)."""
    return 7000 + 131 * c.D + 17 * c.Nq + 3 * c.Nk + 5 * c.B + c.H + (1 if c.ps else 0) + (2 if c.kind == 'cross' else 0)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def kt2_key(Nk):
    """The largest key 128 b + 85 below Nk - 1: second 64 of a 128-key block, second key tile of its wave (-1: there is none)."""
    b = (Nk - 2 - 85) // 128
    return 128 * b + 85 if b >= 0 else -1


def position_pool(Nk):
    pool = []
    for p in (0, 15, 16, 31, 32, 63, 64, Nk - 2, Nk // 2, kt2_key(Nk)):
        if 0 <= p < Nk - 1 and p not in pool:
            pool.append(p)
    return pool


def needle_positions(c, causal=False):
    """-> the needle key of every (batch, head) pair, a list of B * H.  Pair 0 has the last key; with Nk >= 1024 pair 1 has
    kt2_key(Nk); the others walk through position_pool(Nk).  Causal cases: 0, 15, 16 and N - 1."""
    n, Nk = c.B * c.H, c.Nk
    if causal:
        want = [p for p in (Nk - 1, 0, 15, 16) if p < Nk]
        return [want[i % len(want)] for i in range(n)]
    pool = position_pool(Nk)
    fixed = [Nk - 1] + ([kt2_key(Nk)] if Nk >= 1024 else [])
    pool = [p for p in pool if p not in fixed] or [Nk - 1]
    start = 7 * ((c.D // 8 + int(c.ps) + Nk // 64) % 2)
    return (fixed + [pool[(start + i) % len(pool)] for i in range(n)])[:n]


def needle_nats(Nq, Nk):
    """a^2 D^-1/2: NEEDLE_NATS, weakened (module docstring) below 61 keys and for a lone query."""
    return min(NEEDLE_NATS if Nk >= 61 else 1.0 + math.log(Nk), LONE_QUERY_NATS if Nq == 1 else NEEDLE_NATS)


def make_inputs(c, kind='needle', dtype=BF16, causal=False):
    """-> dict(q, k, v, do: what the kernel is given, [B, N, C] in `dtype` (q pre-scaled by D^-1/2 log2 e when c.ps; for a 'self'
    case q, k, v are views of dict['qkv'], [B, N, 3C]); q_ref: the unscaled queries the kernel's arithmetic sees; pos: [B, H] needle
    keys).  kind 'needle' or 'biased' (module docstring).  Callers must not modify the tensors."""
    B, H, Nq, Nk, D = c.B, c.H, c.Nq, c.Nk, c.D
    C = H * D
    g = torch.Generator().manual_seed(case_seed(c))
    rnd = lambda *s: torch.randn(*s, generator=g).to(dtype).double()      # noqa: E731
    q, k, v, do = rnd(B, Nq, H, D), rnd(B, Nk, H, D), rnd(B, Nk, H, D), rnd(B, Nq, C)
    u = torch.randn(H, D, generator=g).double()
    u[:, 0] = 0
    u = u / u.norm(dim=1, keepdim=True)
    a = math.sqrt(needle_nats(Nq, Nk) * math.sqrt(D))
    pos = torch.tensor(needle_positions(c, causal)).view(B, H)
    bi, hi = torch.arange(B).view(B, 1).expand(B, H), torch.arange(H).view(1, H).expand(B, H)
    q = q - (q * u).sum(-1, keepdim=True) * u + a * u          # the random part of q is orthogonal to u_h: see the module docstring
    k[bi, pos, hi] = a * u[hi]
    v[bi, pos, hi] = 4 * v[bi, pos, hi]
    if kind == 'biased':
        beta = math.sqrt(BIAS_NATS * math.sqrt(D))
        q[..., 0] = beta
        k[..., 0] = -beta
    else:
        assert kind == 'needle', kind
    cs = D ** -0.5 * LOG2E
    k, v = k.reshape(B, Nk, C).to(dtype), v.reshape(B, Nk, C).to(dtype)
    qs = (q.reshape(B, Nq, C).float() * cs).to(dtype) if c.ps else q.reshape(B, Nq, C).to(dtype)
    q_ref = (qs.float() / cs).double() if c.ps else qs.double()          # as test_self_attention_prescaled_queries builds it
    out = dict(do=do.to(dtype), q_ref=q_ref, pos=pos)
    if c.kind == 'self':
        out['qkv'] = torch.cat([qs, k, v], -1)
        out['q'], out['k'], out['v'] = out['qkv'][..., :C], out['qkv'][..., C:2 * C], out['qkv'][..., 2 * C:]
    else:
        out['kv'] = torch.cat([k, v], -1)
        out['q'], out['k'], out['v'] = qs, out['kv'][..., :C], out['kv'][..., C:]
    return out


# ---- reference ---------------------------------------------------------------------------------------------------------------------
MUTATIONS = ('drop', 'double', 'mask_last', 'swap_v')       # need two keys or more; 'zero_row' (forward, biased input) needs one


def _heads(t, H):
    B, N, C = t.shape
    return t.reshape(B, N, H, C // H).transpose(1, 2)


def attn_ref64(q, k, v, do, heads, pos=None, causal=False, mutation=None, grads=True):
    """fp64 softmax(q k^T D^-1/2) v per head and its gradients (torch autograd) -> dict(o, dq, dk, dv: [B, N, C]; lse2: [B, H, Nq],
    log2 of the row sums of exp(score); share: [B, H, Nq], the softmax weight of key pos[b, h]).
    mutation (a reference made wrong on purpose): 'drop' the needle key is masked; 'double' it is counted twice; 'mask_last' key Nk - 1
    is masked; 'swap_v' the value rows of the needle and of its neighbour are swapped; 'zero_row' one all-zero key / value row is
    appended."""
    H = heads
    qr, kr, vr = (t.detach().double().clone().requires_grad_(grads) for t in (q, k, v))
    qh, kh, vh = _heads(qr, H), _heads(kr, H), _heads(vr, H)
    B, _, Nq, D = qh.shape
    Nk = kh.shape[2]
    bias = torch.zeros(B, H, Nk, dtype=F64)
    bi, hi = torch.arange(B).view(B, 1).expand(B, H), torch.arange(H).view(1, H).expand(B, H)
    if mutation == 'drop':
        bias[bi, hi, pos] = float('-inf')
    elif mutation == 'double':
        bias[bi, hi, pos] = math.log(2.0)
    elif mutation == 'mask_last':
        bias[:, :, Nk - 1] = float('-inf')
    elif mutation == 'swap_v':
        other = torch.where(pos + 1 < Nk, pos + 1, pos - 1)
        idx = torch.arange(Nk).view(1, 1, Nk).repeat(B, H, 1)
        idx[bi, hi, pos], idx[bi, hi, other] = other, pos
        vh = torch.gather(vh, 2, idx.unsqueeze(-1).expand(B, H, Nk, D))
    elif mutation == 'zero_row':
        kh, vh, bias = F.pad(kh, (0, 0, 0, 1)), F.pad(vh, (0, 0, 0, 1)), F.pad(bias, (0, 1))
    else:
        assert mutation is None, mutation
    s = qh @ kh.transpose(-1, -2) * D ** -0.5 + bias.unsqueeze(2)
    if causal:
        s = s + torch.full((Nq, s.shape[-1]), float('-inf'), dtype=F64).triu(1)
    p = torch.softmax(s, -1)
    o = (p @ vh).transpose(1, 2).reshape(B, Nq, H * D)
    out = dict(o=o.detach(), lse2=torch.logsumexp(s.detach(), -1) * LOG2E)
    if pos is not None:
        out['share'] = torch.gather(p.detach(), 3, pos.view(B, H, 1, 1).expand(B, H, Nq, 1)).squeeze(-1)
    if grads:
        o.backward(do.double())
        out.update(dq=qr.grad, dk=kr.grad, dv=vr.grad)
    return out


# ---- the rounding the kernels are allowed ------------------------------------------------------------------------------------------
def _bf(t):
    return t.to(BF16).float()


def attn_emulated(q, k, v, do, heads, ps=False, grads=True):
    """The algorithm of attn_q_kernel / attn_dkdv_kernel in fp32 on the CPU (module docstring): q, k, v, do as the kernel is given
    them (bf16; q pre-scaled when ps) -> dict(o, lse2, dq, dk, dv), the outputs rounded to bf16."""
    H = heads
    qh, kh, vh, doh = (_heads(t.float(), H) for t in (q, k, v, do))
    B, _, Nq, D = qh.shape
    Nk = kh.shape[2]
    ones = is_ones(D)
    scale = torch.tensor(D, dtype=F32).rsqrt().item()
    s2 = qh @ kh.transpose(-1, -2)
    if not ps:
        s2 = s2 * (scale * LOG2E)
    m = torch.full((B, H, Nq), float('-inf'))
    l, o = torch.zeros(B, H, Nq), torch.zeros(B, H, Nq, D)
    for k0 in range(0, Nk, 64):
        st = s2[..., k0:k0 + 64]
        tmax = st.amax(-1)
        # the test `any lane's maximum > m + 8` is wave-wide: the 16 queries of a tile move their running maxima together
        trig = F.pad(tmax > m + 8.0, (0, -Nq % 16)).view(B, H, -1, 16).any(-1, keepdim=True).expand(-1, -1, -1, 16).reshape(B, H, -1)[..., :Nq]
        mn = torch.where(trig, torch.maximum(m, tmax), m)
        alpha = torch.exp2(m - mn)
        l, o, m = l * alpha, o * alpha.unsqueeze(-1), mn
        e = torch.exp2(st - m.unsqueeze(-1))
        pb = _bf(e)
        l = l + (pb if ones else e).sum(-1)
        o = o + pb @ vh[:, :, k0:k0 + 64]
    ob = _bf(o / l.unsqueeze(-1))
    lse = m + torch.log2(l)
    back = lambda t: t.transpose(1, 2).reshape(B, -1, H * D)      # noqa: E731
    out = dict(o=back(ob), lse2=lse)
    if grads:
        delta = (ob * doh).sum(-1)
        p = torch.exp2(s2 - lse.unsqueeze(-1))
        ds = p * (doh @ vh.transpose(-1, -2) - delta.unsqueeze(-1))
        dsb, pb = _bf(ds), _bf(p)
        out['dq'] = back(_bf(scale * (dsb @ kh)))
        out['dv'] = back(_bf(pb.transpose(-1, -2) @ doh))
        out['dk'] = back(_bf((0.6931471805599453 if ps else scale) * (dsb.transpose(-1, -2) @ qh)))
    return out


# ---- metric ------------------------------------------------------------------------------------------------------------------------
ZERO_SCALE = 2.5e-2


def slice_rel_err(got, ref, heads):
    """max over the (batch, head) slices of max|got - ref| / max|ref| inside the slice; [B, N, heads * D] tensors.  A non-finite
    `got` gives inf.  A slice whose reference is identically zero -- dQ and dK of a softmax over ONE key, where dS = P (dP - delta)
    cancels exactly -- is measured against ZERO_SCALE: the kernels' dP and delta are fp32 sums of up to 160 products of size <= 16
    added in different orders, they differ by <= 1e-4, and dQ / dK by <= 1e-3 = 4e-2 * ZERO_SCALE after the sum over 130 queries
    (the emulation reaches 2e-5); a wrong delta or a wrong probability is O(1)."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, f'shape {tuple(got.shape)} vs {tuple(ref.shape)}'
    if not torch.isfinite(got).all():
        return float('inf')
    err = _heads((got - ref).abs(), heads).amax(dim=(2, 3))
    scale = _heads(ref.abs(), heads).amax(dim=(2, 3))
    scale = torch.where(scale < 1e-12, torch.full_like(scale, ZERO_SCALE), scale)
    return (err / scale).max().item()


def close_slices(got, ref, tol, heads, name=''):
    """close() of tests/test_gpu_ops.py inside every (batch, head) slice -> the largest relative error."""
    e = slice_rel_err(got, ref, heads)
    assert e <= tol, f'{name}: per-(batch, head) max err / max|ref| = {e:.3g} > {tol}'
    return e


def lse_err_bits(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, f'shape {tuple(got.shape)} vs {tuple(ref.shape)}'
    return float('inf') if not torch.isfinite(got).all() else (got - ref).abs().max().item()


# ---- a case's inputs and fp64 reference, computed once per process -----------------------------------------------------------------
@functools.lru_cache(maxsize=16)
def case_data(c, kind='needle', dtype=BF16, causal=False, grads=True):
    """(inputs, fp64 reference) of a case: callers must not modify the tensors (plain and checks on the same case share them)."""
    x = make_inputs(c, kind, dtype, causal)
    return x, attn_ref64(x['q_ref'], x['k'], x['v'], x['do'], c.H, pos=x['pos'], causal=causal, grads=grads)


# ---- the measurement behind GRAD_TOL -----------------------------------------------------------------------------------------------
def measure_tolerance(path=None):
    """attn_emulated against attn_ref64 over every gradient case -> {name: largest per-slice error}, written out as a table."""
    worst, rows = {}, {}
    for c in GRAD_CASES:
        x, ref = case_data(c)
        emu = attn_emulated(x['q'], x['k'], x['v'], x['do'], c.H, c.ps)
        e = {n: slice_rel_err(emu[n], ref[n], c.H) for n in ('o', 'dq', 'dk', 'dv')}
        e['lse'] = lse_err_bits(emu['lse2'], ref['lse2'])
        for n, val in e.items():
            if val > worst.get(n, (0, None))[0]:
                worst[n] = (val, case_id(c))
            r = rows.setdefault(c.D, {})
            r[n] = max(r.get(n, 0), val)
    lines = ['attn_emulated (tests/attn_cases.py: the kernels\' rounding, fp32 on the CPU) against the fp64 reference, needle inputs,',
             f'largest per-(batch, head) max|err| / max|ref| over the {len(GRAD_CASES)} gradient cases of tests/attn_cases.py (lse: absolute, log2 domain)', '',
             '   D        o      lse       dq       dk       dv']
    for D in sorted(rows):
        r = rows[D]
        lines.append(f'{D:4d}  {r["o"]:.5f}  {r["lse"]:.5f}  {r["dq"]:.5f}  {r["dk"]:.5f}  {r["dv"]:.5f}')
    lines.append('')
    for n in ('o', 'lse', 'dq', 'dk', 'dv'):
        lines.append(f'largest {n:3s} {worst[n][0]:.5f}  ({worst[n][1]})')
    lines.append('')
    for n in ('dq', 'dk', 'dv'):
        b = min(max(GRAD_TOL_FLOOR, 2 * worst[n][0]), 1.0)
        lines.append(f'bound {n}: max({GRAD_TOL_FLOOR}, 2 x {worst[n][0]:.5f}) = {b:.4f} -> GRAD_TOL[{n!r}] = {GRAD_TOL[n]}   (must stay <= {GRAD_TOL_CEILING})')
    lines.append(f'bound o: FWD_TOL = {FWD_TOL} (the bf16 bound of tests/test_gpu_ops.py); bound lse: LSE_TOL_BITS = {LSE_TOL_BITS}')
    lines += ['', 'tests/test_gpu_attn_widths.py on an MI355X, largest per-slice figure of the whole file (the largest errors sit where kernel and',
              'emulation round the output to the same bf16 number, hence the equal digits):']
    lines += [f'  {n:9s} {v:.5f}  ({where})' for n, (v, where) in MEASURED_MI355X.items()]
    text = '\n'.join(lines) + '\n'
    if path:
        with open(path, 'w') as f:
            f.write(text)
    print(text)
    return {n: w[0] for n, w in worst.items()}


if __name__ == '__main__':
    measure_tolerance(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'attn_needle_tolerance.txt'))
