// Short-key attention core (gfx950), shared by the causal text attention (text.hip) and the two-set image-prompt cross-attention
// (ip_attn.hip): at most 128 keys per set, so the WHOLE key set of a (batch, head) is staged in LDS once and published by one
// barrier, a wave sees all of its keys before it needs a probability (single-pass softmax, exp2 domain, fp32: no running maximum,
// no rescale), and P never leaves the registers.
//
// Orientation as attention.hip / attn_wide.hip: S^T[key][query] = mfma(A = K rows, B = Q rows), whose accumulator (lane: column =
// query, 4 consecutive keys) is the B operand of O^T[d][query] += mfma(A = V^T, B = P^T).  A wave owns 16 queries (lane: query li,
// lane group lg) and works on 16-key sub-tiles j; `nsub` is the number of sub-tiles it visits, the rest are skipped (their scores
// stay -inf), not computed and masked.  The operations are templated on the element type T and the tiled width DP >= D (columns
// D .. DP - 1 of Q, K and V are zeros):
//            K step             staged chunks   staged rows, DP granule (short_tile)   V^T                            P
//   bf16     K = 32 MFMA        8 elements      32: whole 32-key tiles                 tr_frag32 of the V tile        rounded to bf16 once
//   fp32     16x16x4 MFMA       4 elements      16: whole 16-key sub-tiles             the row-major tile, lane = d   fp32
// fp32: k-step r of sub-tile j contracts keys 16 j + 4 lg + r, which is where the accumulator of S^T already holds them.
//
// Host side (below the device code): validation of the [B][N][ld] views and the width dispatcher.
#pragma once
#include "attn_frag.h"
#include <math.h>
#include <initializer_list>
#include <type_traits>

constexpr int SHORT_MAXN = 128;    // most keys of one set: 8 sub-tiles x 4 scores per lane in registers
constexpr int SHORT_MAXSUB = SHORT_MAXN / 16;

template <typename T> constexpr int short_tile() { return sizeof(T) == 2 ? 32 : 16; }
template <typename T> constexpr int short_rows(int n) { return (n + short_tile<T>() - 1) & ~(short_tile<T>() - 1); }
// LDS row stride (elements) of a K / V image: bf16 tile_ld(), fp32 DP + 4
template <typename T, int DP> constexpr int short_ld() {
    static_assert(DP % short_tile<T>() == 0, "DP is a multiple of the element type's tile");
    return sizeof(T) == 2 ? tile_ld<DP>() : DP + 4;
}
// bytes of `rows` staged rows of K and of V (rows: a sum of short_rows())
template <typename T, int DP> constexpr size_t short_lds_bytes(int rows) { return (size_t)2 * rows * short_ld<T, DP>() * sizeof(T); }

#define SHORT_MFMA_F32(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

// K and V of one (batch, head) -> Ks / Vs [rows][LD], by all `nthr` threads of the block; rows past N and columns past D as zeros
template <typename T, int DP>
DEVFN void short_stage(T* Ks, T* Vs, const T* Kg, const T* Vg, int ldk, int ldv, int rows, int N, int D, int tid, int nthr) {
    typedef std::conditional_t<sizeof(T) == 2, bf16x8, f32x4> chunk;         // 16 bytes
    constexpr int LD = short_ld<T, DP>(), CH = 16 / (int)sizeof(T), NCH = DP / CH;
    const chunk z = __builtin_bit_cast(chunk, (u32x4){0u, 0u, 0u, 0u});
    for (int idx = tid; idx < rows * NCH; idx += nthr) {
        const int row = idx / NCH, col = (idx % NCH) * CH;
        const bool in = row < N && col < D;
        *reinterpret_cast<chunk*>(Ks + row * LD + col) = in ? *reinterpret_cast<const chunk*>(Kg + (long long)row * ldk + col) : z;
        *reinterpret_cast<chunk*>(Vs + row * LD + col) = in ? *reinterpret_cast<const chunk*>(Vg + (long long)row * ldv + col) : z;
    }
}

// One 16-query tile's Q rows as B operands.  bf16: lane (li, lg) holds Q[q][32 s + 8 lg .. + 8]; fp32 (x4 form): Q[q][4 k + lg].
template <typename T, int DP>
struct ShortQ {
    static constexpr bool HALF = sizeof(T) == 2;
    static constexpr int NW = HALF ? DP / 32 : DP / 4;
    std::conditional_t<HALF, bf16x8, float> w[NW];
    // qh: the head's first row; a row q >= Nq rereads row 0 (and is not stored)
    DEVFN void load(const T* qh, int q, int Nq, int ldq, int D, int lg) {
        const T* qrow = qh + (long long)(q < Nq ? q : 0) * ldq + lg * (HALF ? 8 : 1);
#pragma unroll
        for (int s = 0; s < NW; s++) {
            if constexpr (HALF) w[s] = s * 32 + lg * 8 < D ? ld8(qrow + s * 32) : zero8();
            else w[s] = 4 * s + lg < D ? qrow[4 * s] : 0.f;
        }
    }
};

// raw scores of the 16-key sub-tile j (lane: query li, keys 16 j + 4 lg .. + 4)
template <typename T, int DP>
DEVFN f32x4 short_qk(const T* Ks, int j, const ShortQ<T, DP>& q, int li, int lg) {
    constexpr int LD = short_ld<T, DP>();
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    if constexpr (sizeof(T) == 2) {
        const bf16* kr = Ks + (16 * j + li) * LD + lg * 8;
#pragma unroll
        for (int ss = 0; ss < DP / 32; ss++)
            s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8*>(kr + ss * 32), q.w[ss], s, 0, 0, 0);
    } else {
        const float* kr = Ks + (16 * j + li) * LD + lg;
#pragma unroll
        for (int k = 0; k < DP / 4; k++) s = SHORT_MFMA_F32(kr[4 * k], q.w[k], s);
    }
    return s;
}

// Scaled and masked scores of one key set: sub-tiles j < nsub are computed, the others stay -inf.  Keys >= N are masked to -inf; CAUSAL:
// only on the diagonal sub-tile nsub - 1 (the one that holds the wave's own queries, and the only visited one that can reach N),
// where keys > qrow (the lane's query) are masked as well.  Key 0 is never masked, so a row's maximum is finite.
template <typename T, int DP, int NSUB, bool CAUSAL>
DEVFN void short_scores(f32x4 (&sc)[NSUB], const T* Ks, const ShortQ<T, DP>& q, int nsub, int N, float scale2, int qrow, int li, int lg) {
#pragma unroll
    for (int j = 0; j < NSUB; j++) {
        sc[j] = (f32x4){-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        if (j < nsub) {                              // wave-uniform
            f32x4 s = short_qk<T, DP>(Ks, j, q, li, lg);
            const int k0 = 16 * j + 4 * lg;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                s[r] *= scale2;
                const bool out = CAUSAL ? j == nsub - 1 && (k0 + r > qrow || k0 + r >= N) : k0 + r >= N;
                if (out) s[r] = -INFINITY;
            }
            sc[j] = s;
        }
    }
}

// single-pass softmax over the NSUB sub-tiles of one set: sc <- exp2(sc - max), returns the row sum
// (FAST: v_exp_f32 directly -- arguments <= 0, a denormal result may flush to 0, far below a bf16 probability's rounding)
template <int NSUB, bool FAST>
DEVFN float short_softmax(f32x4 (&sc)[NSUB]) {
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < NSUB; j++)
#pragma unroll
        for (int r = 0; r < 4; r++) m = fmaxf(m, sc[j][r]);
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    m = fmaxf(m, __shfl_xor(m, 32, 64));             // finite: key 0 is unmasked in every row
    float l = 0.f;
#pragma unroll
    for (int j = 0; j < NSUB; j++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            sc[j][r] = FAST ? __builtin_amdgcn_exp2f(sc[j][r] - m) : exp2f(sc[j][r] - m);      // exp2(-inf) = 0 for masked and skipped keys
            l += sc[j][r];
        }
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    return l;
}

// acc (O^T: lane = query li, channels 16 i + 4 lg .. + 4) += P~ V over the visited sub-tiles.  bf16: per 32-key tile t, visited with
// its sub-tile 2 t (the probabilities of a skipped sub-tile 2 t + 1 are zeros, and its rows are staged).
template <typename T, int DP, int NSUB>
DEVFN void short_pv(f32x4 (&acc)[DP / 16], const T* Vs, const f32x4 (&sc)[NSUB], int nsub, int li, int lg) {
    constexpr int LD = short_ld<T, DP>(), DT = DP / 16;
    if constexpr (sizeof(T) == 2) {
#pragma unroll
        for (int t = 0; t < NSUB / 2; t++) {
            if (2 * t < nsub) {                      // wave-uniform
                const bf16x8 pf = pack_p(sc[2 * t], sc[2 * t + 1]);
#pragma unroll
                for (int i = 0; i < DT; i++)
                    acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag32(Vs, LD, 32 * t, i * 16, li, lg), pf, acc[i], 0, 0, 0);
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < NSUB; j++) {
            if (j < nsub) {                          // wave-uniform
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const float* vr = Vs + (16 * j + 4 * lg + r) * LD + li;      // A[d = 16 i + li][k = lg] = V[key 16 j + 4 lg + r][d]
#pragma unroll
                    for (int i = 0; i < DT; i++) acc[i] = SHORT_MFMA_F32(vr[16 * i], sc[j][r], acc[i]);
                }
            }
        }
    }
}

// orow (the lane's query row of the head) <- acc * inv, rounded once; channels >= D are skipped
template <typename T, int DP>
DEVFN void short_store(T* orow, const f32x4 (&acc)[DP / 16], float inv, int D, int lg) {
#pragma unroll
    for (int i = 0; i < DP / 16; i++) {
        const f32x4 o = acc[i] * inv;
        if (i * 16 + lg * 4 >= D) continue;
        if constexpr (sizeof(T) == 2) *reinterpret_cast<bf16x4*>(orow + i * 16 + lg * 4) = (bf16x4){f2bf(o[0]), f2bf(o[1]), f2bf(o[2]), f2bf(o[3])};
        else *reinterpret_cast<f32x4*>(orow + i * 16 + lg * 4) = o;
    }
}

// ---- host side ----

// One [B][N][ld] view of T: base pointer, token stride and batch stride (elements)
struct AttnView {
    const void* p;
    long long ld, bs;
};
// every view has a 16-byte-aligned base, rows of at least hd = H * D elements, a non-negative batch stride, and strides that keep
// every row 16-byte aligned
template <typename T>
inline bool attn_views_ok(std::initializer_list<AttnView> views, long long hd) {
    constexpr long long EA = 16 / (long long)sizeof(T) - 1;      // elements per 16 bytes, minus one
    for (const AttnView& v : views)
        if (!v.p || ((uintptr_t)v.p & 15) || v.ld < hd || (v.ld & EA) || v.bs < 0 || (v.bs & EA)) return false;
    return true;
}

// f(std::integral_constant<int, DP>) at DP = D rounded up to a multiple of STEP, MAXDP at the most (D is validated by the caller)
template <int STEP, int MAXDP, int DP = STEP, typename F>
int attn_width_dispatch(int D, F&& f) {
    if constexpr (DP >= MAXDP) return f(std::integral_constant<int, MAXDP>{});
    else return D <= DP ? f(std::integral_constant<int, DP>{}) : attn_width_dispatch<STEP, MAXDP, DP + STEP>(D, f);
}
