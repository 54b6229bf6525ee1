"""The inputs of the all-pairs LPIPS layer tests (tests/test_gpu_diversity.py) and the figures their preconditions rest on, which
tests/test_diversity_host.py checks without a GPU.

Recipe for a case (C, ldf, h, wd, G, K) and a seeded generator: per group a base map P = |randn(h, wd, ldf)|; row i of group g is
relu(P + s_i randn) with s_i = 0.05 (1 + 0.5 g) 1.25^i, so the rows of a group are close to each other (as K seeds of one prompt are)
and every pair of a group has its own distance; 20 % of the pixels of every row are all-zero (a ReLU's dead pixels); w = 0.1 rand(C);
the columns past C are NaN when ldf > C (they are not read)."""
import torch

import fidelity_ref as ref

U = 2.0 ** -24
# (C, ldf, h, wd, G, K)
BIT_CASES = [(4, 4, 3, 5, 1, 2), (64, 64, 7, 9, 2, 3), (512, 520, 2, 3, 1, 16), (20, 32, 16, 17, 3, 5), (64, 64, 12, 11, 1, 16), (128, 128, 16, 16, 2, 8)]
FP64_CASES = [(64, 64, 7, 9, 2, 3), (20, 32, 16, 17, 3, 5), (128, 128, 16, 16, 2, 8)]
# the paths the cases above do not reach in the on-chip form: C = 256 and C = 512 (four and eight chunks per lane; the second over
# several pixel blocks with a tail), C > 512 (the chunk loop that is not unrolled), a group whose copy does not fit in LDS, and
# (4, 4, 256, 257): 514 pixel blocks with a tail, the size from which the library itself takes the on-chip form
EXTRA_BIT_CASES = [(256, 256, 5, 7, 2, 4), (512, 512, 12, 11, 1, 3), (576, 580, 2, 3, 1, 3), (576, 576, 1, 2, 1, 8), (4, 4, 256, 257, 1, 3)]


def chip_fits(C, K):
    """The admitted set of the on-chip form (include/sidlsg_hip.h): the K normalised vectors of 128 pixels next to the accumulators in 64 KB."""
    return K * (K - 1) // 2 * 128 + 2048 * K * ((C + 63) // 64) <= 65536


def forms(C, K):
    """The launch forms a case is run in: the library's choice, and each form by name where it is admitted."""
    return (None, 'chip', 'pairs') if chip_fits(C, K) else (None, 'pairs')


def k_bound(C):
    """tests/test_gpu_fidelity.py::test_lpips_layer_against_fp64: 2 L + 18 with L = 4 ceil(C / 64) channels per lane."""
    return 2 * (4 * ((C + 63) // 64)) + 18


def pair_table(K):
    return [(i, j) for i in range(K) for j in range(i + 1, K)]


def rows(C, ldf, h, wd, G, K, gen, first_group=0):
    """-> F [G*K, h, wd, ldf] fp32 by the recipe."""
    out = []
    for g in range(first_group, first_group + G):
        base = torch.randn(h, wd, ldf, generator=gen).abs()
        for i in range(K):
            s = 0.05 * (1 + 0.5 * g) * 1.25 ** i
            out.append(torch.relu(base + s * torch.randn(h, wd, ldf, generator=gen)))
    F = torch.stack(out)
    F[torch.rand(G * K, h, wd, generator=gen) < 0.2] = 0.0
    if ldf > C:
        F[..., C:] = float('nan')
    return F


_made = {}


def make(case):
    """-> (F [G*K, h, wd, ldf], w [C]) on the CPU, seed C + h + K; built once per case and shared (do not write to them)."""
    if case not in _made:
        C, ldf, h, wd, G, K = case
        gen = torch.Generator().manual_seed(C + h + K)
        F = rows(C, ldf, h, wd, G, K, gen)
        _made[case] = (F, 0.1 * torch.rand(C, generator=gen))
    return _made[case]


def gather(F, G, K):
    """The pair list of a grouped buffer, as the paired kernel takes it: [2 G P, ..], rows n and G P + n are pair n (group-major)."""
    table = pair_table(K)
    ia = [g * K + i for g in range(G) for i, _ in table]
    ib = [g * K + j for g in range(G) for _, j in table]
    return torch.cat([F[ia], F[ib]])


_fp64 = {}


def fp64(case):
    """-> (want [G, P], M [G, P]) from fidelity_ref.lpips_layer on the gathered pairs; computed once per case."""
    if case not in _fp64:
        C, ldf, h, wd, G, K = case
        F, w = make(case)
        want, M = ref.lpips_layer(gather(F, G, K), w, C)
        _fp64[case] = (want.reshape(G, -1), M.reshape(G, -1))
    return _fp64[case]


def smallest_gap(case):
    """min over two different pairs of a case of |want_a - want_b| / max(bound_a, bound_b), bound = k(C) 2^-24 M."""
    want, M = fp64(case)
    want, bound = want.reshape(-1), k_bound(case[0]) * U * M.reshape(-1)
    gap = (want[:, None] - want[None, :]).abs() / torch.maximum(bound[:, None], bound[None, :])
    gap.fill_diagonal_(float('inf'))
    return float(gap.min())
