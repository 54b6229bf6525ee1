// CLIP text encoder (gfx950): causal self-attention for short sequences and the token + position embedding.
//
// sidlsg_attn_causal_fwd(_f32): O = softmax(mask(Q K^T D^-1/2)) V per head, key j visible to query i iff j <= i, 1 <= N <= 128
// (CLIP: 77), D a multiple of 8 up to 128 (tiled at DP = D rounded up to 32 for bf16, to 16 for fp32; the pad columns of Q, K and V
// are zeros).  Forward only, no LSE: the text encoder is frozen.
//   - one workgroup per (batch, head); wave w owns queries 16 w .. 16 w + 15, so a block is ceil(N / 16) waves (1 .. 8);
//   - the head's whole K and V are staged in LDS once (rows past N as zeros) and published by ONE barrier: bf16 rows padded to
//     tile_ld() of attention.hip (an odd multiple of 32 bytes), 2 * 128 * 144 * 2 = 72 KB at N = D = 128, 30 KB for CLIP-L (N = 77 ->
//     96 rows of 80); fp32 rows padded to DP + 4, 2 * 80 * 68 * 4 = 43 KB for CLIP-L, 132 KB at the maximum;
//   - wave w visits the 16-key sub-tiles 0 .. w only: the causal half is skipped, not computed and masked.  Only the diagonal
//     sub-tile (and key columns >= N) is masked to -inf, before the row maximum; key 0 is visible to every row, so the maximum is
//     finite and no NaN can arise;
//   - a wave sees all of its keys before it needs any probability: a single-pass softmax (no running maximum, no rescale), exp2
//     domain, fp32.  At most 8 sub-tiles x 4 scores per lane live in registers;
//   - orientation as attn_wide.hip: S^T[key][query] = mfma(A = K rows, B = Q rows), whose accumulator (lane: column = query, 4
//     consecutive keys) is the B operand of O^T[d][query] += mfma(A = V^T, B = P^T) with no LDS round trip for P.  bf16: P rounded to
//     bf16 once, V^T by ds_read_b64_tr_b16 over 32-key tiles.  fp32: v_mfma_f32_16x16x4_f32 throughout, nothing rounded to bf16: k-step
//     r of sub-tile j contracts keys 16 j + 4 g + r (g = lane group), which is where the accumulator of S^T already holds them.
//   - query rows >= N are never stored.
//
// sidlsg_text_embed(_f32): out[b L + l][:] = tok[ids[b][l]][:] + pos[l][:], summed in fp32 and rounded once at the store.  An id
// outside [0, V) reads nothing and writes its row as NaN.
#include "common.h"
#include <math.h>

namespace {

constexpr int CMAXN = 128;         // longest sequence: 8 waves of 16 queries

typedef __attribute__((address_space(3))) s16x4 lds_s16x4_c;

template <typename T>
struct CausalParams {
    const T *Q, *K, *V;
    T* O;
    int H, N, D;                   // D <= DP, the width the kernel is tiled for: columns D .. DP - 1 are staged / loaded as zeros
    int ldq, ldk, ldv, ldo;
    long long bsq, bsk, bsv, bso;
    float scale2;                  // D^-0.5 * log2(e)
};

// LDS row stride (elements) of a bf16 K / V image: the smallest odd multiple of 16 elements >= DP (tile_ld() of attention.hip)
constexpr int causal_ld(int DP) { return (DP / 16) % 2 ? DP : DP + 16; }

// as tr_frag32 of attention.hip: A operand = X^T of rows r0 + {4g..4g+3} and r0 + 16 + {4g..4g+3}, columns c0 .. c0 + 15
DEVFN bf16x8 causal_tr_frag(const bf16* tile, int LD, int r0, int c0, int li, int lg) {
    const bf16* p0 = tile + (r0 + 4 * lg + (li >> 2)) * LD + c0 + (li & 3) * 4;
    const bf16* p1 = p0 + 16 * LD;
    s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_c*)p0);
    s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_c*)p1);
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, v);
}

// scores of the 16-key sub-tile j of wave w (lane: query q, keys k0 .. k0 + 3): scaled, masked where key > query or key >= N
DEVFN void causal_mask(f32x4& s, int j, int w, int k0, int q, int N, float scale2) {
#pragma unroll
    for (int r = 0; r < 4; r++) {
        s[r] *= scale2;
        if (j == w && (k0 + r > q || k0 + r >= N)) s[r] = -INFINITY;
    }
}

template <int DP>
__global__ __launch_bounds__(512) void attn_causal_bf16_kernel(CausalParams<bf16> p) {
    constexpr int LD = causal_ld(DP), NCH = DP / 8, NS = DP / 32, DT = DP / 16;
    extern __shared__ __attribute__((aligned(16))) char smem_c[];
    const int N = p.N, D = p.D;
    const int NR = (N + 31) & ~31;                   // staged rows: whole 32-key tiles
    bf16* Ks = reinterpret_cast<bf16*>(smem_c);      // [NR][LD]
    bf16* Vs = Ks + NR * LD;                         // [NR][LD]
    const int b = blockIdx.x / p.H, h = blockIdx.x % p.H;
    const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, lg = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);      // in an SGPR: the `j <= w` tests below are scalar branches
    const bf16* Kg = p.K + b * p.bsk + h * D;
    const bf16* Vg = p.V + b * p.bsv + h * D;
    for (int idx = tid; idx < NR * NCH; idx += blockDim.x) {
        const int row = idx / NCH, col = (idx % NCH) * 8;
        const bool in = row < N && col < D;
        st8(Ks + row * LD + col, in ? ld8(Kg + (long long)row * p.ldk + col) : zero8());
        st8(Vs + row * LD + col, in ? ld8(Vg + (long long)row * p.ldv + col) : zero8());
    }
    const int q0 = 16 * w, q = q0 + li;
    // Q rows as B operands: lane (li, lg) holds Q[q][32 s + 8 lg .. + 8]; rows >= N of the last wave reread row 0 and are not stored
    bf16x8 qf[NS];
    {
        const bf16* qrow = p.Q + b * p.bsq + h * D + (long long)(q < N ? q : 0) * p.ldq + lg * 8;
#pragma unroll
        for (int s = 0; s < NS; s++) qf[s] = s * 32 + lg * 8 < D ? ld8(qrow + s * 32) : zero8();
    }
    __syncthreads();

    const int nt = w / 2 + 1;                        // 32-key tiles of this wave; sub-tile 2 t + 1 > w of the last one is skipped
    f32x4 sc[4][2];
#pragma unroll
    for (int t = 0; t < 4; t++) {
#pragma unroll
        for (int hh = 0; hh < 2; hh++) {
            const int j = 2 * t + hh;
            sc[t][hh] = (f32x4){-INFINITY, -INFINITY, -INFINITY, -INFINITY};
            if (j <= w) {                            // wave-uniform
                f32x4 s = {0.f, 0.f, 0.f, 0.f};
                const bf16* kr = Ks + (16 * j + li) * LD + lg * 8;
#pragma unroll
                for (int ss = 0; ss < NS; ss++)
                    s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8*>(kr + ss * 32), qf[ss], s, 0, 0, 0);
                causal_mask(s, j, w, 16 * j + 4 * lg, q, N, p.scale2);
                sc[t][hh] = s;
            }
        }
    }
    float m = -INFINITY;
#pragma unroll
    for (int t = 0; t < 4; t++)
#pragma unroll
        for (int hh = 0; hh < 2; hh++)
#pragma unroll
            for (int r = 0; r < 4; r++) m = fmaxf(m, sc[t][hh][r]);
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    m = fmaxf(m, __shfl_xor(m, 32, 64));             // finite: key 0 is unmasked in every row
    float l = 0.f;
#pragma unroll
    for (int t = 0; t < 4; t++)
#pragma unroll
        for (int hh = 0; hh < 2; hh++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                sc[t][hh][r] = exp2f(sc[t][hh][r] - m);      // exp2(-inf) = 0 for masked and skipped keys
                l += sc[t][hh][r];
            }
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);

    f32x4 acc[DT];
#pragma unroll
    for (int i = 0; i < DT; i++) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 4; t++) {
        if (t < nt) {                                // wave-uniform
            const f32x4 a = sc[t][0], c = sc[t][1];
            const bf16x8 pf = {f2bf(a[0]), f2bf(a[1]), f2bf(a[2]), f2bf(a[3]), f2bf(c[0]), f2bf(c[1]), f2bf(c[2]), f2bf(c[3])};
#pragma unroll
            for (int i = 0; i < DT; i++)
                acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(causal_tr_frag(Vs, LD, 32 * t, i * 16, li, lg), pf, acc[i], 0, 0, 0);
        }
    }
    if (q >= N) return;
    const float inv = 1.0f / l;
    bf16* orow = p.O + b * p.bso + h * D + (long long)q * p.ldo + lg * 4;     // lane: query q, channels 16 i + 4 lg .. + 4
#pragma unroll
    for (int i = 0; i < DT; i++) {
        const bf16x4 o = {f2bf(acc[i][0] * inv), f2bf(acc[i][1] * inv), f2bf(acc[i][2] * inv), f2bf(acc[i][3] * inv)};
        if (i * 16 + lg * 4 < D) *reinterpret_cast<bf16x4*>(orow + i * 16) = o;
    }
}

#define MFMA_F32(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

template <int DP>
__global__ __launch_bounds__(512) void attn_causal_f32_kernel(CausalParams<float> p) {
    constexpr int LD = DP + 4, NCH = DP / 4, NK = DP / 4, DT = DP / 16;
    extern __shared__ __attribute__((aligned(16))) char smem_c[];
    const int N = p.N, D = p.D;
    const int NR = (N + 15) & ~15;                   // staged rows: whole 16-key sub-tiles
    float* Ks = reinterpret_cast<float*>(smem_c);    // [NR][LD]
    float* Vs = Ks + NR * LD;                        // [NR][LD]
    const int b = blockIdx.x / p.H, h = blockIdx.x % p.H;
    const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, lg = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);      // in an SGPR: the `j <= w` tests below are scalar branches
    const float* Kg = p.K + b * p.bsk + h * D;
    const float* Vg = p.V + b * p.bsv + h * D;
    const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
    for (int idx = tid; idx < NR * NCH; idx += blockDim.x) {
        const int row = idx / NCH, col = (idx % NCH) * 4;
        const bool in = row < N && col < D;
        *reinterpret_cast<f32x4*>(Ks + row * LD + col) = in ? *reinterpret_cast<const f32x4*>(Kg + (long long)row * p.ldk + col) : z4;
        *reinterpret_cast<f32x4*>(Vs + row * LD + col) = in ? *reinterpret_cast<const f32x4*>(Vg + (long long)row * p.ldv + col) : z4;
    }
    const int q0 = 16 * w, q = q0 + li;
    // Q rows as B operands of the x4 form: lane (li, lg) holds Q[q][4 k + lg]
    float qf[NK];
    {
        const float* qrow = p.Q + b * p.bsq + h * D + (long long)(q < N ? q : 0) * p.ldq + lg;
#pragma unroll
        for (int k = 0; k < NK; k++) qf[k] = 4 * k + lg < D ? qrow[4 * k] : 0.f;
    }
    __syncthreads();

    f32x4 sc[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
        sc[j] = (f32x4){-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        if (j <= w) {                                // wave-uniform
            f32x4 s = {0.f, 0.f, 0.f, 0.f};
            const float* kr = Ks + (16 * j + li) * LD + lg;
#pragma unroll
            for (int k = 0; k < NK; k++) s = MFMA_F32(kr[4 * k], qf[k], s);
            causal_mask(s, j, w, 16 * j + 4 * lg, q, N, p.scale2);
            sc[j] = s;
        }
    }
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < 8; j++)
#pragma unroll
        for (int r = 0; r < 4; r++) m = fmaxf(m, sc[j][r]);
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    float l = 0.f;
#pragma unroll
    for (int j = 0; j < 8; j++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            sc[j][r] = exp2f(sc[j][r] - m);
            l += sc[j][r];
        }
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);

    f32x4 acc[DT];
#pragma unroll
    for (int i = 0; i < DT; i++) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 8; j++) {
        if (j <= w) {                                // wave-uniform
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const float* vr = Vs + (16 * j + 4 * lg + r) * LD + li;      // A[d = 16 i + li][k = lg] = V[key 16 j + 4 lg + r][d]
#pragma unroll
                for (int i = 0; i < DT; i++) acc[i] = MFMA_F32(vr[16 * i], sc[j][r], acc[i]);
            }
        }
    }
    if (q >= N) return;
    const float inv = 1.0f / l;
    float* orow = p.O + b * p.bso + h * D + (long long)q * p.ldo + lg * 4;
#pragma unroll
    for (int i = 0; i < DT; i++)
        if (i * 16 + lg * 4 < D) *reinterpret_cast<f32x4*>(orow + i * 16) = (f32x4){acc[i][0] * inv, acc[i][1] * inv, acc[i][2] * inv, acc[i][3] * inv};
}

template <typename T>
size_t causal_lds_bytes(int N, int DP) {
    if (sizeof(T) == 2) return (size_t)2 * ((N + 31) & ~31) * causal_ld(DP) * 2;
    return (size_t)2 * ((N + 15) & ~15) * (DP + 4) * 4;
}

template <typename T, int DP>
int launch_causal(const CausalParams<T>& p, int B, hipStream_t s) {
    const void* fn;
    if constexpr (sizeof(T) == 2) fn = reinterpret_cast<const void*>(&attn_causal_bf16_kernel<DP>);
    else fn = reinterpret_cast<const void*>(&attn_causal_f32_kernel<DP>);
    static bool attr_done = false;                   // per instantiation: the largest image this (T, DP) can ask for
    if (!attr_done) {
        if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)causal_lds_bytes<T>(CMAXN, DP)) != hipSuccess)
            return (int)hipGetLastError();
        attr_done = true;
    }
    const size_t lds = causal_lds_bytes<T>(p.N, DP);
    const dim3 grid((unsigned)(B * p.H)), block((unsigned)(64 * ((p.N + 15) / 16)));
    SidlsgTraceScope ts(SIDLSG_FAM_ATTN_FWD, 2.0 * B * p.H * (double)p.N * p.N * p.D, 4.0 * sizeof(T) * B * p.H * (double)p.N * p.D);
    if constexpr (sizeof(T) == 2) SIDLSG_LAUNCH(attn_causal_bf16_kernel<DP>, grid, block, lds, s, p);
    else SIDLSG_LAUNCH(attn_causal_f32_kernel<DP>, grid, block, lds, s, p);
    return sidlsg_last_error();
}

template <typename T>
int attn_causal_t(const void* Q, const void* K, const void* V, void* O, int B, int H, int N, int D, int ldq, int ldk, int ldv, int ldo,
                  long long bsq, long long bsk, long long bsv, long long bso, void* stream) {
    constexpr int EA = 16 / (int)sizeof(T) - 1;      // elements per 16 bytes, minus one
    if (!Q || !K || !V || !O || B <= 0 || H <= 0 || N < 1 || N > CMAXN) return SIDLSG_EINVAL;
    if (D < 8 || D > 128 || (D & 7)) return SIDLSG_EINVAL;
    if ((long long)B * H >= (1LL << 31)) return SIDLSG_EINVAL;
    const long long hd = (long long)H * D;
    if (ldq < hd || ldk < hd || ldv < hd || ldo < hd || ((ldq | ldk | ldv | ldo) & EA)) return SIDLSG_EINVAL;
    if (bsq < 0 || bsk < 0 || bsv < 0 || bso < 0 || ((bsq | bsk | bsv | bso) & EA)) return SIDLSG_EINVAL;
    if (((uintptr_t)Q | (uintptr_t)K | (uintptr_t)V | (uintptr_t)O) & 15) return SIDLSG_EINVAL;
    CausalParams<T> p;
    p.Q = (const T*)Q; p.K = (const T*)K; p.V = (const T*)V; p.O = (T*)O;
    p.H = H; p.N = N; p.D = D; p.ldq = ldq; p.ldk = ldk; p.ldv = ldv; p.ldo = ldo; p.bsq = bsq; p.bsk = bsk; p.bsv = bsv; p.bso = bso;
    p.scale2 = (float)(1.4426950408889634 / sqrt((double)D));
    hipStream_t s = (hipStream_t)stream;
    if constexpr (sizeof(T) == 2) {
        switch ((D + 31) / 32) {
            case 1: return launch_causal<T, 32>(p, B, s);
            case 2: return launch_causal<T, 64>(p, B, s);
            case 3: return launch_causal<T, 96>(p, B, s);
            default: return launch_causal<T, 128>(p, B, s);
        }
    } else {
        switch ((D + 15) / 16) {
            case 1: return launch_causal<T, 16>(p, B, s);
            case 2: return launch_causal<T, 32>(p, B, s);
            case 3: return launch_causal<T, 48>(p, B, s);
            case 4: return launch_causal<T, 64>(p, B, s);
            case 5: return launch_causal<T, 80>(p, B, s);
            case 6: return launch_causal<T, 96>(p, B, s);
            case 7: return launch_causal<T, 112>(p, B, s);
            default: return launch_causal<T, 128>(p, B, s);
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void text_embed_kernel(const long long* __restrict__ ids, const float* __restrict__ tok,
                                                         const float* __restrict__ pos, T* __restrict__ out, int rows, int L, int D, int V) {
    const int nch = D >> 3;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)rows * nch) return;
    const int row = (int)(idx / nch), c = (int)(idx % nch) * 8;
    const long long id = ids[row];
    float v[8];
    if (id < 0 || id >= V) {                         // nothing is read for an id outside the table; the row is loud instead
#pragma unroll
        for (int e = 0; e < 8; e++) v[e] = __builtin_nanf("");
    } else {
        float t[8], q[8];
        ldv8<float>(tok + id * D + c, t);
        ldv8<float>(pos + (long long)(row % L) * D + c, q);
#pragma unroll
        for (int e = 0; e < 8; e++) v[e] = t[e] + q[e];
    }
    stv8<T>(out + (long long)row * D + c, v);
}

template <typename T>
int text_embed_t(const void* ids, const float* tok, const float* pos, void* out, int B, int L, int D, int V, int P, void* stream) {
    if (!ids || !tok || !pos || !out || B <= 0 || L <= 0 || D <= 0 || V <= 0 || P <= 0 || L > P || (D & 7)) return SIDLSG_EINVAL;
    if (((uintptr_t)tok | (uintptr_t)pos | (uintptr_t)out) & 15 || ((uintptr_t)ids & 7)) return SIDLSG_EINVAL;
    const long long rows = (long long)B * L, n = rows * (D >> 3);
    if (rows * D >= (1LL << 31)) return SIDLSG_EINVAL;
    hipLaunchKernelGGL(text_embed_kernel<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const long long*)ids, tok,
                       pos, (T*)out, (int)rows, L, D, V);
    return sidlsg_last_error();
}

}  // namespace

extern "C" {

int sidlsg_attn_causal_fwd(const void* Q, const void* K, const void* V, void* O, int B, int H, int N, int D, int ldq, int ldk, int ldv,
                           int ldo, long long bsq, long long bsk, long long bsv, long long bso, void* stream) {
    return attn_causal_t<bf16>(Q, K, V, O, B, H, N, D, ldq, ldk, ldv, ldo, bsq, bsk, bsv, bso, stream);
}
int sidlsg_attn_causal_fwd_f32(const void* Q, const void* K, const void* V, void* O, int B, int H, int N, int D, int ldq, int ldk, int ldv,
                               int ldo, long long bsq, long long bsk, long long bsv, long long bso, void* stream) {
    return attn_causal_t<float>(Q, K, V, O, B, H, N, D, ldq, ldk, ldv, ldo, bsq, bsk, bsv, bso, stream);
}

int sidlsg_text_embed(const void* ids, const float* tok, const float* pos, void* out, int B, int L, int D, int V, int P, void* stream) {
    return text_embed_t<bf16>(ids, tok, pos, out, B, L, D, V, P, stream);
}
int sidlsg_text_embed_f32(const void* ids, const float* tok, const float* pos, void* out, int B, int L, int D, int V, int P, void* stream) {
    return text_embed_t<float>(ids, tok, pos, out, B, L, D, V, P, stream);
}

}  // extern "C"
