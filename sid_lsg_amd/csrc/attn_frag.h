// bf16 MFMA fragment helpers shared by the attention kernels (attention.hip, attn_wide.hip, and attn_short.h for text.hip and
// ip_attn.hip): the row stride of a staged LDS tile, the transposed A-operand read of it, and the B operand packed from two
// accumulator tiles.
#pragma once
#include "common.h"

typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

// LDS tile of ROWS rows with a row stride of LD = the smallest odd multiple of 16 elements >= DP (32 B x odd): with that
// stride both the ds_read_b128 fragment reads (16-lane groups of the b128 access) and the ds_read_b64_tr_b16 transpose reads
// (32-lane halves) touch every bank slot exactly once -- brute-forced over the access patterns of attention.hip; the former
// DP + 8 stride was 2-way conflicted on both (SQ_LDS_BANK_CONFLICT = 45 % of SQ_LDS_IDX_ACTIVE, profiles/r02_attn_pmc.json).
// Columns DP..LD (when LD > DP) are never read.  The over-read of the K=32 slices (DP = 16, 48, 80: LD == DP) runs into
// the NEXT row's first 16 columns (finite data, multiplied by the global operand's exact zeros) and, for the last row, into
// 16 elements of slack that are zeroed once per block (lds_tile_init() of attention.hip).
template <int DP>
constexpr int tile_ld() { return ((DP + 15) / 16) % 2 ? (DP + 15) / 16 * 16 : (DP + 15) / 16 * 16 + 16; }

// A operand = X^T for a row-major LDS tile X[row][LD]: rows r0 + {4g..4g+3} and r0 + 16 + {4g..4g+3},
// columns c0..c0+15 -> lane i gets column c0+i, the 8 rows in the order that matches pack_p().
DEVFN bf16x8 tr_frag32(const bf16* tile, int LD, int r0, int c0, int li, int lg) {
    const bf16* p0 = tile + (r0 + 4 * lg + (li >> 2)) * LD + c0 + (li & 3) * 4;
    const bf16* p1 = p0 + 16 * LD;
    s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)p0);
    s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)p1);
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, v);
}
// two accumulator tiles (rows 0-15 and 16-31 of the contraction index) -> one K=32 B operand
DEVFN bf16x8 pack_p(f32x4 a, f32x4 b) {
    bf16x8 o = {f2bf(a[0]), f2bf(a[1]), f2bf(a[2]), f2bf(a[3]), f2bf(b[0]), f2bf(b[1]), f2bf(b[2]), f2bf(b[3])};
    return o;
}
