"""Per-prompt diversity: how different the K images are that one prompt yields under K seeds.

The measure is the mean pairwise LPIPS among the K samples of one condition (intra-prompt diversity).  Precision / recall cannot see a
generator whose pictures vary across the set but are near-identical per prompt; this can.  `HipLPIPS.group_pairs` runs VGG16 once per
image and forms all K (K - 1) / 2 pairs of a group on chip (sidlsg_lpips_group_f32), each value the bits `HipLPIPS(a_i, a_j)` gives;
SSIM and the squared error of the same pairs come from the existing one-pass kernel on the gathered pair list.

This module holds the host rules: the pair order, the per-group figures and the figures of a set.  generate_onestep.py --diversity,
tools/prompt_diversity.py and the `lpipsdiv*` metrics share them.
"""
import math

import torch

from . import fidelity

SSIM_BATCH = 4096          # pairs per psnr_ssim call (the kernel admits 21845)


def pair_index(K):
    """-> [K (K - 1) / 2, 2] int64: the pairs (i, j), i < j, in lexicographic order -- the order of sidlsg_lpips_group_f32's outputs."""
    if K < 2:
        raise ValueError(f'pair_index: a group of {K} has no pair')
    return torch.tensor([(i, j) for i in range(K) for j in range(i + 1, K)], dtype=torch.int64)


def check_group_size(K, what='--seeds_per_prompt'):
    if not 2 <= K <= fidelity.GROUP_MAX:
        raise ValueError(f'{what} {K}: diversity is scored over groups of 2 .. {fidelity.GROUP_MAX} images')


def score_groups(images_u8, K, lpips):
    """uint8 [G*K, 3, H, W] on the device, group g = images gK .. gK+K-1 -> one dict per group: `lpips` (the mean of the pair values,
    added in pair order in fp64), `lpips_min`, `lpips_pairs` (the K (K - 1) / 2 values in pair_index order), and `ssim` / `mse`, the
    means over the same pairs."""
    N = images_u8.shape[0]
    if N % K:
        raise ValueError(f'score_groups: {N} images are not whole groups of {K}')
    G = N // K
    table = pair_index(K)
    P = table.shape[0]
    lp = lpips.group_pairs(images_u8, K).cpu().tolist()
    base = torch.arange(G, dtype=torch.int64)[:, None] * K
    ia, ib = (base + table[None, :, 0]).reshape(-1).to(images_u8.device), (base + table[None, :, 1]).reshape(-1).to(images_u8.device)
    rows = []
    for s in range(0, G * P, SSIM_BATCH):
        rows += fidelity.psnr_ssim(images_u8[ia[s:s + SSIM_BATCH]].contiguous(), images_u8[ib[s:s + SSIM_BATCH]].contiguous())
    out = []
    for g in range(G):
        pairs, own = lp[g], rows[g * P:(g + 1) * P]
        total = 0.0
        for v in pairs:
            total += v
        out.append(dict(lpips=total / P, lpips_min=min(pairs), lpips_pairs=pairs, ssim=sum(r['ssim'] for r in own) / P,
                        mse=sum(r['mse'] for r in own) / P))
    return out


def aggregate(per_prompt):
    """The figures of a set from its per-group dicts (a list, or a dict keyed by group): `groups`, the means over groups of `lpips`,
    `lpips_min`, `ssim` and `mse`, and `lpips_std`, the population standard deviation of `lpips` over groups."""
    rows = list(per_prompt.values()) if isinstance(per_prompt, dict) else list(per_prompt)
    if not rows:
        raise ValueError('aggregate: no groups')
    n = len(rows)
    out = {'groups': n}
    for key in ('lpips', 'lpips_min', 'ssim', 'mse'):
        out[key] = sum(r[key] for r in rows) / n
    out['lpips_std'] = math.sqrt(sum((r['lpips'] - out['lpips']) ** 2 for r in rows) / n)
    return out


def format_means(mean):
    return (f'{mean["groups"]} groups: lpips {mean["lpips"]:.6g} (std over groups {mean["lpips_std"]:.6g}), lpips_min {mean["lpips_min"]:.6g}, '
            f'ssim {mean["ssim"]:.6g}, mse {mean["mse"]:.6g}')


def groups_of(keys, K):
    """Sample keys (the index that picks a sample's condition: key // K) -> {group: [keys]} in key order; every group must be whole."""
    groups = {}
    for k in sorted(keys):
        groups.setdefault(k // K, []).append(k)
    bad = {g: v for g, v in groups.items() if len(v) != K}
    if bad:
        g, v = next(iter(bad.items()))
        raise ValueError(f'the samples do not form whole groups of {K}: condition {g} has {len(v)} sample(s) ({v})')
    return groups
