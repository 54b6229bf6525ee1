"""Shared by tests/test_ip_cases_host.py and tests/test_gpu_ip_adapter.py (not a test module): needle inputs for the two-set
cross-attention of csrc/ip_attn.hip, their fp64 reference, references made wrong on purpose, and a CPU emulation of the rounding the
kernel is allowed.  The recipe is that of tests/attn_cases.py, whose helpers it imports.

    O = softmax(q K^T D^-1/2) V  +  s * softmax(q K2^T D^-1/2) V2        (K, V: the text set, Nk keys; K2, V2: the image set, Nk2 keys)

Inputs.  q, K, V, K2, V2 are bf16 randn (fp32 randn for the fp32 kernel).  One unit vector u_h per head with u_h[0] = 0; every query's
own component along u_h is replaced by a u_h, a^2 D^-1/2 = needle_nats(Nq, Nk).  Every (batch, head) pair has ONE needle key in each set:
K[j] = a u_h (score needle_nats(Nq, Nk)) and K2[j2] = a2 u_h with a a2 D^-1/2 = needle_nats(Nq, Nk2), i.e. 1 + ln Nk2 nats for the
short image set.  Pair 0 has its image needle at key Nk2 - 1 and its text needle at Nk - 1; the positions rotate over the pairs.
Kinds: 'image' -- the image needle's V2 row is x 4, the text needle's V row is not, so what happens to the image set decides the output;
'text' -- the other way round; 'biased' -- the 'image' kind with column 0 of q set to + beta and column 0 of K AND K2 to - beta,
beta^2 D^-1/2 = 12: both softmaxes are unchanged, and a phantom all-zero key that escaped the mask of either set would weigh e^12 real
ones.

Mutations of the reference (`mutation`, applied to the set named by `target`): 'drop' the needle key is masked (a set of one key then
contributes nothing); 'double' it is counted twice; 'mask_last' the set's last key is masked; 'swap_v' the value rows of the needle and
of its neighbour are swapped; 'other_row' the set's keys and values are those of the next batch row; 'no_scale' s is ignored (taken as
1); 'joint' ONE softmax over the union of both sets (s applied to the image values); 'zero_row' a phantom all-zero key / value row is
appended to the set (biased kind).  mutations_for() lists the ones that change anything for a case: with Nk2 = 1 'double' and 'swap_v'
do not exist, and 'no_scale' needs s != 1.

cross2_emulated: the kernel's algorithm in fp32 on the CPU -- per set a single-pass softmax in the exp2 domain, the un-normalised
probabilities exp2(score - max) rounded to bf16 in front of the PV contraction, acc = P2 V2, acc *= s l / l2, acc += P V, O = acc / l,
rounded to bf16 once.  It models the rounding this project tolerates; it is not the code under test.

Bound: FWD_TOL = 1.2e-2 of max |ref| inside every (batch, head) slice (close_slices of tests/attn_cases.py); the fp32 kernel 2e-5.
"""
import collections
import functools
import math

import torch

from attn_cases import BIAS_NATS, FWD_TOL, close_slices, needle_nats, slice_rel_err  # noqa: F401  (re-exported to the tests)

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
LOG2E = 1.4426950408889634
F32_TOL = 2e-5               # the fp32 attention bound of tests/test_gpu_fp32.py, per slice

Case2 = collections.namedtuple('Case2', 'B H Nq Nk Nk2 D ps')
KINDS = ('image', 'text')
SET_MUTATIONS = ('drop', 'double', 'mask_last', 'swap_v', 'other_row')      # apply to either set
IMAGE_ONLY_MUTATIONS = ('no_scale', 'joint')

HOST_CASES = tuple(Case2(2, 4, 130, 77, nk2, D, False) for nk2 in (1, 4, 16, 17) for D in (8, 40, 64, 80, 160))
HOST_SCALES = (1.0, 0.5)
GPU_WIDTHS = (8, 16, 40, 64, 80, 128, 160)
GPU_SHAPES = ((130, 77, 4), (130, 77, 1), (130, 77, 16), (130, 77, 17), (130, 77, 32), (1, 77, 4), (17, 13, 4), (130, 128, 4), (130, 1, 4))
GPU_BIASED_NK2 = (4, 17)


def case_id(c):
    return f'd{c.D}-q{c.Nq}k{c.Nk}i{c.Nk2}-b{c.B}h{c.H}' + ('-ps' if c.ps else '')


def case_seed(c):
    """One seed per case: a fixed function of its numbers (never of anything measured)."""
    return 9000 + 131 * c.D + 17 * c.Nq + 3 * c.Nk + 29 * c.Nk2 + 5 * c.B + c.H + (1 if c.ps else 0)


def _rotate(n, N, start=0):
    """Needle keys of n pairs in a set of N keys: pair 0 the last key, the others walk through 0, 15, 16, N // 2, N - 2."""
    pool = []
    for p in (0, 15, 16, N // 2, N - 2, 31, 32, 63, 64):
        if 0 <= p < N - 1 and p not in pool:
            pool.append(p)
    pool = pool or [N - 1]
    return ([N - 1] + [pool[(start + i) % len(pool)] for i in range(n)])[:n]


def make_inputs(c, kind='image', dtype=BF16):
    """-> dict(q, k, v, k2, v2: what the kernel is given, [B, N, H * D] in `dtype` (q pre-scaled by D^-1/2 log2 e when c.ps); q_ref: the
    unscaled queries the kernel's arithmetic sees (fp64); pos, pos2: [B, H] needle keys of the two sets).  Callers must not modify them."""
    B, H, Nq, Nk, Nk2, D = c.B, c.H, c.Nq, c.Nk, c.Nk2, c.D
    C = H * D
    g = torch.Generator().manual_seed(case_seed(c))
    rnd = lambda *s: torch.randn(*s, generator=g).to(dtype).double()      # noqa: E731
    q, k, v, k2, v2 = rnd(B, Nq, H, D), rnd(B, Nk, H, D), rnd(B, Nk, H, D), rnd(B, Nk2, H, D), rnd(B, Nk2, H, D)
    u = torch.randn(H, D, generator=g).double()
    u[:, 0] = 0
    u = u / u.norm(dim=1, keepdim=True)
    a = math.sqrt(needle_nats(Nq, Nk) * math.sqrt(D))
    a2 = needle_nats(Nq, Nk2) * math.sqrt(D) / a
    pos = torch.tensor(_rotate(B * H, Nk, start=c.D // 8 % 2)).view(B, H)
    pos2 = torch.tensor(_rotate(B * H, Nk2)).view(B, H)
    bi, hi = torch.arange(B).view(B, 1).expand(B, H), torch.arange(H).view(1, H).expand(B, H)
    q = q - (q * u).sum(-1, keepdim=True) * u + a * u
    k[bi, pos, hi] = a * u[hi]
    k2[bi, pos2, hi] = a2 * u[hi]
    base = 'image' if kind == 'biased' else kind
    assert base in KINDS, kind
    if base == 'image':
        v2[bi, pos2, hi] = 4 * v2[bi, pos2, hi]
    else:
        v[bi, pos, hi] = 4 * v[bi, pos, hi]
    if kind == 'biased':
        beta = math.sqrt(BIAS_NATS * math.sqrt(D))
        q[..., 0] = beta
        k[..., 0] = -beta
        k2[..., 0] = -beta
    cs = D ** -0.5 * LOG2E
    flat = lambda t: t.reshape(t.shape[0], t.shape[1], C).to(dtype)       # noqa: E731
    qs = (q.reshape(B, Nq, C).float() * cs).to(dtype) if c.ps else flat(q)
    q_ref = (qs.float() / cs).double() if c.ps else qs.double()
    return dict(q=qs, k=flat(k), v=flat(v), k2=flat(k2), v2=flat(v2), q_ref=q_ref, pos=pos, pos2=pos2)


def mutations_for(c, s, target, kind):
    """The mutations that change the result of a case (module docstring)."""
    n = c.Nk2 if target == 'image' else c.Nk
    if kind == 'biased':
        return ('zero_row',)
    out = [m for m in SET_MUTATIONS if n > 1 or m in ('drop', 'mask_last', 'other_row')]
    if target == 'image':
        out += [m for m in IMAGE_ONLY_MUTATIONS if m != 'no_scale' or s != 1]
    return tuple(out)


# ---- reference ---------------------------------------------------------------------------------------------------------------------
def _heads(t, H):
    B, N, C = t.shape
    return t.reshape(B, N, H, C // H).transpose(1, 2)


def _set_scores(qh, kh, vh, pos, mutation):
    """One set's scores [B, H, Nq, N'] (fp64, with the mutation's bias), and its possibly mutated values."""
    B, H, _, D = qh.shape
    N = kh.shape[2]
    bias = torch.zeros(B, H, N, dtype=F64)
    bi, hi = torch.arange(B).view(B, 1).expand(B, H), torch.arange(H).view(1, H).expand(B, H)
    if mutation == 'drop':
        bias[bi, hi, pos] = float('-inf')
    elif mutation == 'double':
        bias[bi, hi, pos] = math.log(2.0)
    elif mutation == 'mask_last':
        bias[:, :, N - 1] = float('-inf')
    elif mutation == 'swap_v':
        other = torch.where(pos + 1 < N, pos + 1, pos - 1)
        idx = torch.arange(N).view(1, 1, N).repeat(B, H, 1)
        idx[bi, hi, pos], idx[bi, hi, other] = other, pos
        vh = torch.gather(vh, 2, idx.unsqueeze(-1).expand(B, H, N, D))
    elif mutation == 'other_row':
        kh, vh = kh.roll(1, 0), vh.roll(1, 0)
    elif mutation == 'zero_row':
        kh, vh, bias = torch.nn.functional.pad(kh, (0, 0, 0, 1)), torch.nn.functional.pad(vh, (0, 0, 0, 1)), torch.nn.functional.pad(bias, (0, 1))
    else:
        assert mutation is None, mutation
    return qh @ kh.transpose(-1, -2) * D ** -0.5 + bias.unsqueeze(2), vh


def cross2_ref64(x, s, heads, mutation=None, target='image'):
    """fp64 reference [B, Nq, C] of the inputs `x` (make_inputs) at scale s; `mutation` on the set `target` makes it wrong on purpose."""
    H = heads
    qh = _heads(x['q_ref'].double(), H)
    kh, vh, k2h, v2h = (_heads(x[n].double(), H) for n in ('k', 'v', 'k2', 'v2'))
    B, _, Nq, D = qh.shape
    mt = mutation if target == 'text' and mutation not in IMAGE_ONLY_MUTATIONS else None
    mi = mutation if target == 'image' and mutation not in IMAGE_ONLY_MUTATIONS else None
    s1, vh = _set_scores(qh, kh, vh, x['pos'], mt)
    s2, v2h = _set_scores(qh, k2h, v2h, x['pos2'], mi)
    if mutation == 'no_scale':
        s = 1.0
    if mutation == 'joint':
        p = torch.softmax(torch.cat([s1, s2], -1), -1)
        o = p[..., :s1.shape[-1]] @ vh + s * (p[..., s1.shape[-1]:] @ v2h)
    else:
        o = torch.nan_to_num(torch.softmax(s1, -1), nan=0.0) @ vh + s * (torch.nan_to_num(torch.softmax(s2, -1), nan=0.0) @ v2h)
    return o.transpose(1, 2).reshape(B, Nq, H * D)


def one_set_ref64(x, heads):
    """fp64 softmax(q K^T D^-1/2) V of the text set alone: what s = 0 must give."""
    return cross2_ref64(x, 0.0, heads)


# ---- the rounding the kernel is allowed ----------------------------------------------------------------------------------------------
def _bf(t):
    return t.to(BF16).float()


def cross2_emulated(x, s, heads, ps=False):
    """The algorithm of attn_cross2_kernel<bf16> in fp32 on the CPU (module docstring) -> [B, Nq, C], rounded to bf16."""
    H = heads
    qh, kh, vh, k2h, v2h = (_heads(x[n].float(), H) for n in ('q', 'k', 'v', 'k2', 'v2'))
    B, _, Nq, D = qh.shape
    sc = 1.0 if ps else torch.tensor(D, dtype=F32).rsqrt().item() * LOG2E

    def probs(kk):
        t = qh @ kk.transpose(-1, -2) * sc
        e = torch.exp2(t - t.amax(-1, keepdim=True))
        return _bf(e), e.sum(-1, keepdim=True)

    p1, l1 = probs(kh)
    o = torch.zeros(1)
    if s != 0:
        p2, l2 = probs(k2h)
        o = (p2 @ v2h) * (float(s) * l1 / l2)
    o = (o + p1 @ vh) / l1
    return _bf(o).transpose(1, 2).reshape(B, Nq, H * D)


# ---- a case's inputs and fp64 reference, computed once per process -----------------------------------------------------------------
@functools.lru_cache(maxsize=64)
def case_inputs(c, kind='image', dtype=BF16):
    return make_inputs(c, kind, dtype)


@functools.lru_cache(maxsize=64)
def case_ref(c, kind, s, dtype=BF16):
    return cross2_ref64(case_inputs(c, kind, dtype), s, c.H)
