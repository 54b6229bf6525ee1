// Decoupled cross-attention of an image-prompt adapter (gfx950): two key sets, two softmaxes, ONE launch.
//
// sidlsg_attn_cross2_fwd(_ps, _f32):  O = softmax(Q K^T D^-1/2) V + s * softmax(Q K2^T D^-1/2) V2  per head.  The first set is the
// text (1 <= Nk <= 128 keys, 77 for SD), the second the image tokens (1 <= Nk2 <= 32, 4 for the published SD 1.5 adapters); any
// Nq >= 1.  bf16: D a multiple of 8 up to 160, tiled at DP = D rounded up to 32; fp32: D a multiple of 4 up to 160, tiled at
// DP = D rounded up to 16; the pad columns of Q, K and V are zeros.  Forward only, no LSE: the adapter runs in sampling passes.
//   - a workgroup is 8 waves and owns `tpb` consecutive 16-query tiles of one (batch, head); wave w takes tiles w, w + 8, ... and
//     requests the next tile's Q rows before it starts on the current one;
//   - both key sets of the (batch, head) are staged in LDS once per workgroup (rows past Nk / Nk2 as zeros) and published by ONE
//     barrier: bf16 rows padded to an odd multiple of 32 bytes as in text.hip, (128 + 32) * 176 * 2 * 2 = 110 KB at the maximum,
//     41 KB for SD's 77 + 4 keys at D = 40 (96 + 32 rows of 80), 90 KB at D = 160; fp32 rows padded to DP + 4.  K / V are re-staged per
//     workgroup and the staging is what a short launch waits for, so a workgroup is as large as the hardware allows: tpb = 8 (128
//     queries, one tile per wave) below 2048 queries, 32 (512 queries) from there on.  Measured at SD 1.5's shapes (B 16, H 8, 77 + 4
//     keys; profiles/ip_adapter.txt): 4 waves with tpb 4 / 16 took 45 / 37 / 25 / 11 us at (Nq, D) = (4096, 40) / (1024, 80) /
//     (256, 160) / (64, 160), 8 waves take 39 / 21 / 12 / 11 us;
//   - a wave sees all keys of a set before it needs a probability: a single-pass softmax per set (no running maximum, no rescale),
//     exp2 domain, fp32.  Key columns >= Nk (>= Nk2) are masked to -inf before the row maximum; key 0 of either set is never
//     masked, so both maxima are finite.  At most (8 + 2) sub-tiles x 4 scores per lane live in registers;
//   - each set is normalised on its own, and both share ONE fp32 accumulator: acc = P2~ V2 (P~ = exp2(score - max), un-normalised, so
//     the largest probability of a row is exactly 1), acc *= s l / l2, acc += P~ V, O = acc / l -- the sum is rounded once, at the
//     store.  bf16: P~ is rounded to bf16 once in front of the PV contraction; fp32: nothing is rounded to bf16;
//   - orientation as text.hip / attn_wide.hip: S^T[key][query] = mfma(A = K rows, B = Q rows), whose accumulator (lane: column =
//     query, 4 consecutive keys) is the B operand of O^T[d][query] += mfma(A = V^T, B = P^T) with no LDS round trip for P; V^T by
//     ds_read_b64_tr_b16 over 32-key tiles (bf16), v_mfma_f32_16x16x4_f32 throughout (fp32);
//   - s == 0 skips the image set altogether: K2 / V2 are not read, and the result is the one-set attention of this kernel;
//   - query rows >= Nq are never stored.
#include "common.h"
#include <math.h>

namespace {

constexpr int X2_MAXN = 128;       // text keys
constexpr int X2_MAXN2 = 32;       // image keys: one 32-key tile
constexpr int X2_WAVES = 8;
constexpr size_t X2_LDS_MAX = 160 * 1024;

typedef __attribute__((address_space(3))) s16x4 lds_s16x4_x;

template <typename T>
struct Cross2Params {
    const T *Q, *K, *V, *K2, *V2;
    T* O;
    int H, Nq, Nk, Nk2, D;         // D <= DP, the width the kernel is tiled for: columns D .. DP - 1 are staged / loaded as zeros
    int tpb, nchunk;               // 16-query tiles per workgroup; workgroups per (batch, head)
    int ldq, ldk, ldv, ldk2, ldv2, ldo;
    long long bsq, bsk, bsv, bsk2, bsv2, bso;
    float scale2;                  // D^-0.5 * log2(e); 1 for pre-scaled queries
    float s;
};

// LDS row stride (elements) of a bf16 K / V image: the smallest odd multiple of 16 elements >= DP (causal_ld() of text.hip)
constexpr int x2_ld(int DP) { return (DP / 16) % 2 ? DP : DP + 16; }

// as causal_tr_frag of text.hip: A operand = X^T of rows r0 + {4g..4g+3} and r0 + 16 + {4g..4g+3}, columns c0 .. c0 + 15
DEVFN bf16x8 x2_tr_frag(const bf16* tile, int LD, int r0, int c0, int li, int lg) {
    const bf16* p0 = tile + (r0 + 4 * lg + (li >> 2)) * LD + c0 + (li & 3) * 4;
    const bf16* p1 = p0 + 16 * LD;
    s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_x*)p0);
    s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_x*)p1);
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, v);
}

// scores of one 16-key sub-tile (lane: keys k0 .. k0 + 3): scaled; keys >= N masked
DEVFN void x2_mask(f32x4& s, int k0, int N, float scale2) {
#pragma unroll
    for (int r = 0; r < 4; r++) {
        s[r] *= scale2;
        if (k0 + r >= N) s[r] = -INFINITY;
    }
}

// single-pass softmax over the NSUB sub-tiles of one set (skipped sub-tiles hold -inf): sc <- exp2(sc - max), returns the row sum
// (FAST: v_exp_f32 directly -- arguments <= 0, a denormal result may flush to 0, far below a bf16 probability's rounding)
template <int NSUB, bool FAST>
DEVFN float x2_softmax(f32x4 (&sc)[NSUB]) {
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

template <int DP>
__global__ __launch_bounds__(64 * X2_WAVES) void attn_cross2_bf16_kernel(Cross2Params<bf16> p) {
    constexpr int LD = x2_ld(DP), NCH = DP / 8, NS = DP / 32, DT = DP / 16;
    extern __shared__ __attribute__((aligned(16))) char smem_x[];
    const int Nq = p.Nq, Nk = p.Nk, Nk2 = p.Nk2, D = p.D;
    const int NR = (Nk + 31) & ~31;                  // staged text rows: whole 32-key tiles
    const bool img = p.s != 0.f;                     // uniform
    bf16* Ks = reinterpret_cast<bf16*>(smem_x);      // [NR][LD]
    bf16* Vs = Ks + NR * LD;                         // [NR][LD]
    bf16* K2s = Vs + NR * LD;                        // [32][LD]
    bf16* V2s = K2s + X2_MAXN2 * LD;                 // [32][LD]
    const int bh = blockIdx.x / p.nchunk, chunk = blockIdx.x % p.nchunk;
    const int b = bh / p.H, h = bh % p.H;
    const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, lg = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    {
        const bf16* Kg = p.K + b * p.bsk + h * D;
        const bf16* Vg = p.V + b * p.bsv + h * D;
        for (int idx = tid; idx < NR * NCH; idx += 64 * X2_WAVES) {
            const int row = idx / NCH, col = (idx % NCH) * 8;
            const bool in = row < Nk && col < D;
            st8(Ks + row * LD + col, in ? ld8(Kg + (long long)row * p.ldk + col) : zero8());
            st8(Vs + row * LD + col, in ? ld8(Vg + (long long)row * p.ldv + col) : zero8());
        }
    }
    if (img) {
        const bf16* Kg = p.K2 + b * p.bsk2 + h * D;
        const bf16* Vg = p.V2 + b * p.bsv2 + h * D;
        for (int idx = tid; idx < X2_MAXN2 * NCH; idx += 64 * X2_WAVES) {
            const int row = idx / NCH, col = (idx % NCH) * 8;
            const bool in = row < Nk2 && col < D;
            st8(K2s + row * LD + col, in ? ld8(Kg + (long long)row * p.ldk2 + col) : zero8());
            st8(V2s + row * LD + col, in ? ld8(Vg + (long long)row * p.ldv2 + col) : zero8());
        }
    }
    __syncthreads();

    const int ntiles = (Nq + 15) >> 4;
    const int t_end = min((chunk + 1) * p.tpb, ntiles);
    // Q rows as B operands: lane (li, lg) holds Q[q][32 s + 8 lg .. + 8]; rows >= Nq of the last tile reread row 0 and are not stored.
    // The next tile's rows are requested before this tile's arithmetic, so a wave's tiles do not each expose a global-load latency.
    const bf16* qbase = p.Q + b * p.bsq + h * D + lg * 8;
    bf16x8 qf[NS], qn[NS];
#pragma unroll
    for (int s = 0; s < NS; s++) qn[s] = zero8();
    {
        const int q = (chunk * p.tpb + w) * 16 + li;
        const bf16* qrow = qbase + (long long)(q < Nq ? q : 0) * p.ldq;
#pragma unroll
        for (int s = 0; s < NS; s++) qf[s] = s * 32 + lg * 8 < D ? ld8(qrow + s * 32) : zero8();
    }
    for (int tile = chunk * p.tpb + w; tile < t_end; tile += X2_WAVES) {
        const int q = tile * 16 + li;
        if (tile + X2_WAVES < t_end) {               // uniform
            const int qq = (tile + X2_WAVES) * 16 + li;
            const bf16* qrow = qbase + (long long)(qq < Nq ? qq : 0) * p.ldq;
#pragma unroll
            for (int s = 0; s < NS; s++) qn[s] = s * 32 + lg * 8 < D ? ld8(qrow + s * 32) : zero8();
        }
        f32x4 sc[8], sc2[2];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            sc[j] = (f32x4){-INFINITY, -INFINITY, -INFINITY, -INFINITY};
            if (16 * j < Nk) {                       // uniform
                f32x4 s = {0.f, 0.f, 0.f, 0.f};
                const bf16* kr = Ks + (16 * j + li) * LD + lg * 8;
#pragma unroll
                for (int ss = 0; ss < NS; ss++)
                    s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8*>(kr + ss * 32), qf[ss], s, 0, 0, 0);
                x2_mask(s, 16 * j + 4 * lg, Nk, p.scale2);
                sc[j] = s;
            }
        }
        const float l = x2_softmax<8, true>(sc);
        float l2 = 1.f;
        if (img) {
#pragma unroll
            for (int j = 0; j < 2; j++) {
                sc2[j] = (f32x4){-INFINITY, -INFINITY, -INFINITY, -INFINITY};
                if (16 * j < Nk2) {                  // uniform
                    f32x4 s = {0.f, 0.f, 0.f, 0.f};
                    const bf16* kr = K2s + (16 * j + li) * LD + lg * 8;
#pragma unroll
                    for (int ss = 0; ss < NS; ss++)
                        s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8*>(kr + ss * 32), qf[ss], s, 0, 0, 0);
                    x2_mask(s, 16 * j + 4 * lg, Nk2, p.scale2);
                    sc2[j] = s;
                }
            }
            l2 = x2_softmax<2, true>(sc2);
        }

        f32x4 acc[DT];
#pragma unroll
        for (int i = 0; i < DT; i++) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (img) {                                   // the image set first: its sum is brought to the text set's normalisation
            const f32x4 a = sc2[0], c = sc2[1];
            const bf16x8 pf = {f2bf(a[0]), f2bf(a[1]), f2bf(a[2]), f2bf(a[3]), f2bf(c[0]), f2bf(c[1]), f2bf(c[2]), f2bf(c[3])};
            const float f = p.s * l / l2;
#pragma unroll
            for (int i = 0; i < DT; i++) {
                acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x2_tr_frag(V2s, LD, 0, i * 16, li, lg), pf, acc[i], 0, 0, 0);
                acc[i] *= f;
            }
        }
#pragma unroll
        for (int t = 0; t < 4; t++) {
            if (32 * t < Nk) {                       // uniform
                const f32x4 a = sc[2 * t], c = sc[2 * t + 1];
                const bf16x8 pf = {f2bf(a[0]), f2bf(a[1]), f2bf(a[2]), f2bf(a[3]), f2bf(c[0]), f2bf(c[1]), f2bf(c[2]), f2bf(c[3])};
#pragma unroll
                for (int i = 0; i < DT; i++)
                    acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x2_tr_frag(Vs, LD, 32 * t, i * 16, li, lg), pf, acc[i], 0, 0, 0);
            }
        }
        if (q < Nq) {
            const float inv = 1.0f / l;
            bf16* orow = p.O + b * p.bso + h * D + (long long)q * p.ldo + lg * 4;     // lane: query q, channels 16 i + 4 lg .. + 4
#pragma unroll
            for (int i = 0; i < DT; i++) {
                const bf16x4 o = {f2bf(acc[i][0] * inv), f2bf(acc[i][1] * inv), f2bf(acc[i][2] * inv), f2bf(acc[i][3] * inv)};
                if (i * 16 + lg * 4 < D) *reinterpret_cast<bf16x4*>(orow + i * 16) = o;
            }
        }
#pragma unroll
        for (int ss = 0; ss < NS; ss++) qf[ss] = qn[ss];
    }
}

#define X2_MFMA_F32(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

template <int DP>
__global__ __launch_bounds__(64 * X2_WAVES) void attn_cross2_f32_kernel(Cross2Params<float> p) {
    constexpr int LD = DP + 4, NCH = DP / 4, NK = DP / 4, DT = DP / 16;
    extern __shared__ __attribute__((aligned(16))) char smem_x[];
    const int Nq = p.Nq, Nk = p.Nk, Nk2 = p.Nk2, D = p.D;
    const int NR = (Nk + 15) & ~15, NR2 = (Nk2 + 15) & ~15;      // staged rows: whole 16-key sub-tiles
    const bool img = p.s != 0.f;                     // uniform
    float* Ks = reinterpret_cast<float*>(smem_x);    // [NR][LD]
    float* Vs = Ks + NR * LD;                        // [NR][LD]
    float* K2s = Vs + NR * LD;                       // [NR2][LD]
    float* V2s = K2s + NR2 * LD;                     // [NR2][LD]
    const int bh = blockIdx.x / p.nchunk, chunk = blockIdx.x % p.nchunk;
    const int b = bh / p.H, h = bh % p.H;
    const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, lg = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
    {
        const float* Kg = p.K + b * p.bsk + h * D;
        const float* Vg = p.V + b * p.bsv + h * D;
        for (int idx = tid; idx < NR * NCH; idx += 64 * X2_WAVES) {
            const int row = idx / NCH, col = (idx % NCH) * 4;
            const bool in = row < Nk && col < D;
            *reinterpret_cast<f32x4*>(Ks + row * LD + col) = in ? *reinterpret_cast<const f32x4*>(Kg + (long long)row * p.ldk + col) : z4;
            *reinterpret_cast<f32x4*>(Vs + row * LD + col) = in ? *reinterpret_cast<const f32x4*>(Vg + (long long)row * p.ldv + col) : z4;
        }
    }
    if (img) {
        const float* Kg = p.K2 + b * p.bsk2 + h * D;
        const float* Vg = p.V2 + b * p.bsv2 + h * D;
        for (int idx = tid; idx < NR2 * NCH; idx += 64 * X2_WAVES) {
            const int row = idx / NCH, col = (idx % NCH) * 4;
            const bool in = row < Nk2 && col < D;
            *reinterpret_cast<f32x4*>(K2s + row * LD + col) = in ? *reinterpret_cast<const f32x4*>(Kg + (long long)row * p.ldk2 + col) : z4;
            *reinterpret_cast<f32x4*>(V2s + row * LD + col) = in ? *reinterpret_cast<const f32x4*>(Vg + (long long)row * p.ldv2 + col) : z4;
        }
    }
    __syncthreads();

    const int ntiles = (Nq + 15) >> 4;
    const int t_end = min((chunk + 1) * p.tpb, ntiles);
    for (int tile = chunk * p.tpb + w; tile < t_end; tile += X2_WAVES) {
        const int q = tile * 16 + li;
        // Q rows as B operands of the x4 form: lane (li, lg) holds Q[q][4 k + lg]
        float qf[NK];
        {
            const float* qrow = p.Q + b * p.bsq + h * D + (long long)(q < Nq ? q : 0) * p.ldq + lg;
#pragma unroll
            for (int k = 0; k < NK; k++) qf[k] = 4 * k + lg < D ? qrow[4 * k] : 0.f;
        }
        f32x4 sc[8], sc2[2];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            sc[j] = (f32x4){-INFINITY, -INFINITY, -INFINITY, -INFINITY};
            if (16 * j < Nk) {                       // uniform
                f32x4 s = {0.f, 0.f, 0.f, 0.f};
                const float* kr = Ks + (16 * j + li) * LD + lg;
#pragma unroll
                for (int k = 0; k < NK; k++) s = X2_MFMA_F32(kr[4 * k], qf[k], s);
                x2_mask(s, 16 * j + 4 * lg, Nk, p.scale2);
                sc[j] = s;
            }
        }
        const float l = x2_softmax<8, false>(sc);
        float l2 = 1.f;
        if (img) {
#pragma unroll
            for (int j = 0; j < 2; j++) {
                sc2[j] = (f32x4){-INFINITY, -INFINITY, -INFINITY, -INFINITY};
                if (16 * j < Nk2) {                  // uniform
                    f32x4 s = {0.f, 0.f, 0.f, 0.f};
                    const float* kr = K2s + (16 * j + li) * LD + lg;
#pragma unroll
                    for (int k = 0; k < NK; k++) s = X2_MFMA_F32(kr[4 * k], qf[k], s);
                    x2_mask(s, 16 * j + 4 * lg, Nk2, p.scale2);
                    sc2[j] = s;
                }
            }
            l2 = x2_softmax<2, false>(sc2);
        }

        f32x4 acc[DT];
#pragma unroll
        for (int i = 0; i < DT; i++) acc[i] = z4;
        if (img) {                                   // the image set first: its sum is brought to the text set's normalisation
#pragma unroll
            for (int j = 0; j < 2; j++) {
                if (16 * j < Nk2) {                  // uniform
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const float* vr = V2s + (16 * j + 4 * lg + r) * LD + li;     // A[d = 16 i + li][k = lg] = V2[key 16 j + 4 lg + r][d]
#pragma unroll
                        for (int i = 0; i < DT; i++) acc[i] = X2_MFMA_F32(vr[16 * i], sc2[j][r], acc[i]);
                    }
                }
            }
            const float f = p.s * l / l2;
#pragma unroll
            for (int i = 0; i < DT; i++) acc[i] *= f;
        }
#pragma unroll
        for (int j = 0; j < 8; j++) {
            if (16 * j < Nk) {                       // uniform
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const float* vr = Vs + (16 * j + 4 * lg + r) * LD + li;
#pragma unroll
                    for (int i = 0; i < DT; i++) acc[i] = X2_MFMA_F32(vr[16 * i], sc[j][r], acc[i]);
                }
            }
        }
        if (q < Nq) {
            const float inv = 1.0f / l;
            float* orow = p.O + b * p.bso + h * D + (long long)q * p.ldo + lg * 4;
#pragma unroll
            for (int i = 0; i < DT; i++)
                if (i * 16 + lg * 4 < D) *reinterpret_cast<f32x4*>(orow + i * 16) = acc[i] * inv;
        }
    }
}

template <typename T>
size_t x2_lds_bytes(int Nk, int Nk2, int DP) {
    if (sizeof(T) == 2) return (size_t)2 * (((Nk + 31) & ~31) + X2_MAXN2) * x2_ld(DP) * 2;
    return (size_t)2 * (((Nk + 15) & ~15) + ((Nk2 + 15) & ~15)) * (DP + 4) * 4;
}

template <typename T, int DP>
int launch_cross2(const Cross2Params<T>& p, int B, hipStream_t s) {
    const size_t lds = x2_lds_bytes<T>(p.Nk, p.Nk2, DP);
    if (lds > X2_LDS_MAX) return SIDLSG_EINVAL;      // fp32 only: the bf16 maximum is 110 KB
    const void* fn;
    if constexpr (sizeof(T) == 2) fn = reinterpret_cast<const void*>(&attn_cross2_bf16_kernel<DP>);
    else fn = reinterpret_cast<const void*>(&attn_cross2_f32_kernel<DP>);
    static bool attr_done = false;                   // per instantiation: the largest image this (T, DP) can ask for
    if (!attr_done) {
        const size_t most = x2_lds_bytes<T>(X2_MAXN, X2_MAXN2, DP);
        if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(most < X2_LDS_MAX ? most : X2_LDS_MAX)) != hipSuccess)
            return (int)hipGetLastError();
        attr_done = true;
    }
    const dim3 grid((unsigned)((long long)B * p.H * p.nchunk)), block(64 * X2_WAVES);
    SidlsgTraceScope ts(SIDLSG_FAM_ATTN_FWD, 4.0 * B * p.H * (double)p.Nq * (p.Nk + p.Nk2) * p.D,
                        sizeof(T) * B * p.H * (2.0 * p.Nq + 2.0 * p.Nk + 2.0 * p.Nk2) * p.D);
    if constexpr (sizeof(T) == 2) SIDLSG_LAUNCH(attn_cross2_bf16_kernel<DP>, grid, block, lds, s, p);
    else SIDLSG_LAUNCH(attn_cross2_f32_kernel<DP>, grid, block, lds, s, p);
    return sidlsg_last_error();
}

template <typename T>
int attn_cross2_t(const void* Q, const void* K, const void* V, const void* K2, const void* V2, void* O, float sc, bool prescaled, int B, int H,
                  int Nq, int Nk, int Nk2, int D, int ldq, int ldk, int ldv, int ldk2, int ldv2, int ldo, long long bsq, long long bsk,
                  long long bsv, long long bsk2, long long bsv2, long long bso, void* stream) {
    constexpr int EA = 16 / (int)sizeof(T) - 1;      // elements per 16 bytes, minus one
    constexpr int DSTEP = sizeof(T) == 2 ? 8 : 4;
    if (!Q || !K || !V || !K2 || !V2 || !O || B <= 0 || H <= 0 || Nq < 1) return SIDLSG_EINVAL;
    if (Nk < 1 || Nk > X2_MAXN || Nk2 < 1 || Nk2 > X2_MAXN2) return SIDLSG_EINVAL;
    if (D < DSTEP || D > 160 || D % DSTEP) return SIDLSG_EINVAL;
    if (!(sc == sc) || sc - sc != 0.f) return SIDLSG_EINVAL;                     // NaN or infinite scale
    const long long hd = (long long)H * D;
    if (ldq < hd || ldk < hd || ldv < hd || ldk2 < hd || ldv2 < hd || ldo < hd || ((ldq | ldk | ldv | ldk2 | ldv2 | ldo) & EA)) return SIDLSG_EINVAL;
    if (bsq < 0 || bsk < 0 || bsv < 0 || bsk2 < 0 || bsv2 < 0 || bso < 0 || ((bsq | bsk | bsv | bsk2 | bsv2 | bso) & EA)) return SIDLSG_EINVAL;
    if (((uintptr_t)Q | (uintptr_t)K | (uintptr_t)V | (uintptr_t)K2 | (uintptr_t)V2 | (uintptr_t)O) & 15) return SIDLSG_EINVAL;
    const int ntiles = (int)(((long long)Nq + 15) >> 4);
    Cross2Params<T> p;
    p.tpb = ntiles >= 128 ? 4 * X2_WAVES : X2_WAVES;
    p.nchunk = (ntiles + p.tpb - 1) / p.tpb;
    if ((long long)B * H * p.nchunk >= (1LL << 31)) return SIDLSG_EINVAL;
    p.Q = (const T*)Q; p.K = (const T*)K; p.V = (const T*)V; p.K2 = (const T*)K2; p.V2 = (const T*)V2; p.O = (T*)O;
    p.H = H; p.Nq = Nq; p.Nk = Nk; p.Nk2 = Nk2; p.D = D;
    p.ldq = ldq; p.ldk = ldk; p.ldv = ldv; p.ldk2 = ldk2; p.ldv2 = ldv2; p.ldo = ldo;
    p.bsq = bsq; p.bsk = bsk; p.bsv = bsv; p.bsk2 = bsk2; p.bsv2 = bsv2; p.bso = bso;
    p.scale2 = prescaled ? 1.0f : (float)(1.4426950408889634 / sqrt((double)D));
    p.s = sc;
    hipStream_t s = (hipStream_t)stream;
    if constexpr (sizeof(T) == 2) {
        switch ((D + 31) / 32) {
            case 1: return launch_cross2<T, 32>(p, B, s);
            case 2: return launch_cross2<T, 64>(p, B, s);
            case 3: return launch_cross2<T, 96>(p, B, s);
            case 4: return launch_cross2<T, 128>(p, B, s);
            default: return launch_cross2<T, 160>(p, B, s);
        }
    } else {
        switch ((D + 15) / 16) {
            case 1: return launch_cross2<T, 16>(p, B, s);
            case 2: return launch_cross2<T, 32>(p, B, s);
            case 3: return launch_cross2<T, 48>(p, B, s);
            case 4: return launch_cross2<T, 64>(p, B, s);
            case 5: return launch_cross2<T, 80>(p, B, s);
            case 6: return launch_cross2<T, 96>(p, B, s);
            case 7: return launch_cross2<T, 112>(p, B, s);
            case 8: return launch_cross2<T, 128>(p, B, s);
            case 9: return launch_cross2<T, 144>(p, B, s);
            default: return launch_cross2<T, 160>(p, B, s);
        }
    }
}

}  // namespace

extern "C" {

int sidlsg_attn_cross2_fwd(const void* Q, const void* K, const void* V, const void* K2, const void* V2, void* O, float s, int B, int H, int Nq,
                           int Nk, int Nk2, int D, int ldq, int ldk, int ldv, int ldk2, int ldv2, int ldo, long long bsq, long long bsk,
                           long long bsv, long long bsk2, long long bsv2, long long bso, void* stream) {
    return attn_cross2_t<bf16>(Q, K, V, K2, V2, O, s, false, B, H, Nq, Nk, Nk2, D, ldq, ldk, ldv, ldk2, ldv2, ldo, bsq, bsk, bsv, bsk2, bsv2, bso,
                               stream);
}
int sidlsg_attn_cross2_fwd_ps(const void* Q, const void* K, const void* V, const void* K2, const void* V2, void* O, float s, int B, int H, int Nq,
                              int Nk, int Nk2, int D, int ldq, int ldk, int ldv, int ldk2, int ldv2, int ldo, long long bsq, long long bsk,
                              long long bsv, long long bsk2, long long bsv2, long long bso, void* stream) {
    return attn_cross2_t<bf16>(Q, K, V, K2, V2, O, s, true, B, H, Nq, Nk, Nk2, D, ldq, ldk, ldv, ldk2, ldv2, ldo, bsq, bsk, bsv, bsk2, bsv2, bso,
                               stream);
}
int sidlsg_attn_cross2_fwd_f32(const void* Q, const void* K, const void* V, const void* K2, const void* V2, void* O, float s, int B, int H, int Nq,
                               int Nk, int Nk2, int D, int ldq, int ldk, int ldv, int ldk2, int ldv2, int ldo, long long bsq, long long bsk,
                               long long bsv, long long bsk2, long long bsv2, long long bso, void* stream) {
    return attn_cross2_t<float>(Q, K, V, K2, V2, O, s, false, B, H, Nq, Nk, Nk2, D, ldq, ldk, ldv, ldk2, ldv2, ldo, bsq, bsk, bsv, bsk2, bsv2, bso,
                                stream);
}

}  // extern "C"
