// Precision / recall (Kynkaanniemi et al.; reference metrics/sid_precision_recall.py) on gfx950: pairwise fp16 distances between
// feature sets as one fp16 MFMA contraction whose result never leaves the registers.
//
// Arithmetic, identical in the three entry points (they share pr_tile() and pr_dist()):
//   d2(i, j) = max(|a_i|^2 + |b_j|^2 - 2 a_i . b_j, 0)     a . b on v_mfma_f32_16x16x32_f16, fp32 accumulate; norms in fp32
//   d(i, j)  = fp16_rne(sqrt(d2))                           the reference's distances are fp16 (torch.cdist of fp16 tensors)
// The norms come off the MFMA too: |x|^2 is the diagonal of X X^T, formed from the operand fragments a wave already holds (each wave
// takes 2 of its 4 row blocks and 2 of its 4 column blocks: 4 MFMAs on top of 16).  So each of the three sums is the same chain
// of ceil(F / 32) MFMA accumulations (what the error bound of tests/test_gpu_pr.py is derived from), and a row against itself or
// against a duplicate of itself has |a|^2 = |b|^2 = a . b bit for bit: its distance is exactly 0, the smallest of its row.
//
// One workgroup = 256 threads = 4 waves in 2 x 2, a 128 x 128 tile of (rows x columns), 64 x 64 per wave as 4 x 4 MFMA tiles.
// Both operands are [n][F] row-major, i.e. K-contiguous: each is staged global -> registers -> LDS as a [128][64] fp16 image
// (128-byte rows, the 16-byte chunk index XORed with row & 7) and read back with one ds_read_b128 per MFMA operand.
// LDS is double-buffered over the K steps: the loads of step s + 1 are in flight while step s multiplies; one barrier per step.
// Rows past the end of a set and k past F are staged as zeros; columns past the end never reach a reduction (see the epilogues).
#include "common.h"

typedef _Float16 f16;
typedef f16 f16x8 __attribute__((ext_vector_type(8)));

namespace {

constexpr int PR_T = 128;            // tile edge (rows and columns)
constexpr int PR_BK = 64;            // K elements per step
constexpr int PR_IMG = PR_T * PR_BK * 2;      // bytes of one operand image
constexpr int PR_MAXK1 = 8;          // longest neighbour list: k + 1 <= 8

struct PrSmem {
    unsigned char img[2][2][PR_IMG];      // [buffer][operand: 0 rows, 1 columns]
    float norm[2][PR_T];                  // |.|^2 of the tile's rows / columns
    float list[2][PR_T][PR_MAXK1];        // kth: the two wave columns' lists of every row;  member: [wc][row][0] = flag
};

DEVFN int pr_off(int row, int chunk) { return row * (PR_BK * 2) + ((chunk ^ (row & 7)) << 4); }

// the 4 chunks this thread stages of one operand for K step `k0`
struct PrStage {
    u32x4 v[4];
    DEVFN void load(const f16* __restrict__ X, int n, int F, int r0, int k0, int t) {
        const int k = k0 + ((t & 7) << 3);
#pragma unroll
        for (int p = 0; p < 4; p++) {
            const int row = r0 + (t >> 3) + 32 * p;
            u32x4 q = {0u, 0u, 0u, 0u};
            if (row < n && k < F) q = *reinterpret_cast<const u32x4*>(X + (size_t)row * F + k);
            v[p] = q;
        }
    }
    DEVFN void store(unsigned char* img, int t) const {
#pragma unroll
        for (int p = 0; p < 4; p++) *reinterpret_cast<u32x4*>(img + pr_off((t >> 3) + 32 * p, t & 7)) = v[p];
    }
};

// acc[i][j][r] = rows[row0 + wr*64 + i*16 + (lane>>4)*4 + r] . cols[col0 + wc*64 + j*16 + (lane&15)];  sm.norm = the tile's norms.
// Ends with a barrier: acc and sm.norm are ready, and every wave has left the operand images.
DEVFN void pr_tile(const f16* __restrict__ rows, int R, int row0, const f16* __restrict__ cols, int C, int col0, int F, PrSmem& sm,
                   f32x4 (&acc)[4][4]) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wr = wave >> 1, wc = wave & 1;
    f32x4 na[2], nb[2];      // X X^T blocks of row blocks 2 wc, 2 wc + 1 and column blocks 2 wr, 2 wr + 1 of this wave's quadrant
#pragma unroll
    for (int h = 0; h < 2; h++) na[h] = nb[h] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    PrStage sa, sb;
    const int nk = (F + PR_BK - 1) / PR_BK;
    sa.load(rows, R, F, row0, 0, t);
    sb.load(cols, C, F, col0, 0, t);
    sa.store(sm.img[0][0], t);
    sb.store(sm.img[0][1], t);
    __syncthreads();
    for (int s = 0; s < nk; s++) {
        const int cur = s & 1;
        if (s + 1 < nk) {
            sa.load(rows, R, F, row0, (s + 1) * PR_BK, t);
            sb.load(cols, C, F, col0, (s + 1) * PR_BK, t);
        }
#pragma unroll
        for (int kk = 0; kk < 2; kk++) {
            f16x8 fa[4], fb[4];
            const int chunk = kk * 4 + (lane >> 4);
#pragma unroll
            for (int i = 0; i < 4; i++) {
                fa[i] = *reinterpret_cast<const f16x8*>(sm.img[cur][0] + pr_off(wr * 64 + i * 16 + (lane & 15), chunk));
                fb[i] = *reinterpret_cast<const f16x8*>(sm.img[cur][1] + pr_off(wc * 64 + i * 16 + (lane & 15), chunk));
            }
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 4; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[i], fb[j], acc[i][j], 0, 0, 0);
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const f16x8 xa = wc ? fa[2 + h] : fa[h], xb = wr ? fb[2 + h] : fb[h];
                na[h] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xa, xa, na[h], 0, 0, 0);
                nb[h] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xb, xb, nb[h], 0, 0, 0);
            }
        }
        if (s + 1 < nk) {
            sa.store(sm.img[cur ^ 1][0], t);
            sb.store(sm.img[cur ^ 1][1], t);
        }
        __syncthreads();
    }
    // the diagonal of a 16 x 16 result: column lane & 15 = row (lane >> 4) * 4 + reg
    if (((lane & 15) >> 2) == (lane >> 4)) {
        const int reg = lane & 3;
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const float va = reg == 0 ? na[h][0] : reg == 1 ? na[h][1] : reg == 2 ? na[h][2] : na[h][3];
            const float vb = reg == 0 ? nb[h][0] : reg == 1 ? nb[h][1] : reg == 2 ? nb[h][2] : nb[h][3];
            sm.norm[0][wr * 64 + (2 * wc + h) * 16 + (lane & 15)] = va;
            sm.norm[1][wc * 64 + (2 * wr + h) * 16 + (lane & 15)] = vb;
        }
    }
    __syncthreads();
}

// the fp16 distance, held as the fp32 value of that fp16 number
DEVFN float pr_dist(float na, float nb, float dot) {
    const float d2 = fmaxf(__fmaf_rn(-2.0f, dot, __fadd_rn(na, nb)), 0.0f);
    return (float)(f16)__fsqrt_rn(d2);
}

// keep the K1 smallest of (list, v), ascending; equal values are kept as often as they occur (kthvalue counts multiplicity)
template <int K1> DEVFN void pr_insert(float (&L)[K1], float v) {
#pragma unroll
    for (int q = 0; q < K1; q++) {
        const float lo = fminf(L[q], v);
        v = fmaxf(L[q], v);
        L[q] = lo;
    }
}

__global__ __launch_bounds__(256) void pr_distances_kernel(const f16* __restrict__ rows, int R, const f16* __restrict__ cols, int C, int F,
                                                           f16* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char pr_smem[];
    PrSmem& sm = *reinterpret_cast<PrSmem*>(pr_smem);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wr = wave >> 1, wc = wave & 1;
    const int row0 = blockIdx.y * PR_T, col0 = blockIdx.x * PR_T;
    f32x4 acc[4][4];
    pr_tile(rows, R, row0, cols, C, col0, F, sm, acc);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int cl = wc * 64 + j * 16 + (lane & 15);
        const float nb = sm.norm[1][cl];
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int rl = wr * 64 + i * 16 + (lane >> 4) * 4 + r;
                if (row0 + rl < R && col0 + cl < C) out[(size_t)(row0 + rl) * C + col0 + cl] = (f16)pr_dist(sm.norm[0][rl], nb, acc[i][j][r]);
            }
    }
}

// One workgroup per 128 manifold rows, sweeping every column tile.  Each lane keeps, for each of its 16 accumulator rows, the
// K1 smallest distances it has seen in its columns; the 16 lanes of a row merge by shuffles, the two wave columns through LDS.
template <int K1>
__global__ __launch_bounds__(256) void pr_kth_kernel(const f16* __restrict__ m, int N, int F, int k, f16* __restrict__ radius) {
    extern __shared__ __attribute__((aligned(16))) char pr_smem[];
    PrSmem& sm = *reinterpret_cast<PrSmem*>(pr_smem);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wr = wave >> 1, wc = wave & 1;
    const int row0 = blockIdx.x * PR_T;
    const float INF = __builtin_huge_valf();
    float L[4][4][K1];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int r = 0; r < 4; r++)
#pragma unroll
            for (int q = 0; q < K1; q++) L[i][r][q] = INF;
    for (int col0 = 0; col0 < N; col0 += PR_T) {
        f32x4 acc[4][4];
        pr_tile(m, N, row0, m, N, col0, F, sm, acc);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int cl = wc * 64 + j * 16 + (lane & 15);
            const bool live = col0 + cl < N;
            const float nb = sm.norm[1][cl];
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const float d = pr_dist(sm.norm[0][wr * 64 + i * 16 + (lane >> 4) * 4 + r], nb, acc[i][j][r]);
                    pr_insert<K1>(L[i][r], live ? d : INF);       // a column past the end is never a neighbour
                }
        }
    }
    // the 16 lanes that hold one row (same lane >> 4): butterfly over lane bits 0..3; every lane ends with the row's list
#pragma unroll
    for (int o = 1; o < 16; o <<= 1)
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                float other[K1];
#pragma unroll
                for (int q = 0; q < K1; q++) other[q] = __shfl_xor(L[i][r][q], o, 64);
#pragma unroll
                for (int q = 0; q < K1; q++) pr_insert<K1>(L[i][r], other[q]);
            }
    if ((lane & 15) == 0) {
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int r = 0; r < 4; r++)
#pragma unroll
                for (int q = 0; q < K1; q++) sm.list[wc][wr * 64 + i * 16 + (lane >> 4) * 4 + r][q] = L[i][r][q];
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (t < PR_T && row0 + t < N) {
        float M[K1];
#pragma unroll
        for (int q = 0; q < K1; q++) M[q] = sm.list[0][t][q];
#pragma unroll
        for (int q = 0; q < K1; q++) pr_insert<K1>(M, sm.list[1][t][q]);
        float v = M[0];
#pragma unroll
        for (int q = 1; q < K1; q++) v = (q == k) ? M[q] : v;
        radius[row0 + t] = (f16)v;
    }
}

// inside[i] = any_j d(i, j) <= radius[j]: one workgroup per 128 probes, sweeping every column tile of the manifold.
__global__ __launch_bounds__(256) void pr_member_kernel(const f16* __restrict__ probes, int P, const f16* __restrict__ m, int N, int F,
                                                        const f16* __restrict__ radius, uint8_t* __restrict__ inside) {
    extern __shared__ __attribute__((aligned(16))) char pr_smem[];
    PrSmem& sm = *reinterpret_cast<PrSmem*>(pr_smem);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wr = wave >> 1, wc = wave & 1;
    const int row0 = blockIdx.x * PR_T;
    unsigned flags = 0u;         // bit 4 i + r
    for (int col0 = 0; col0 < N; col0 += PR_T) {
        f32x4 acc[4][4];
        pr_tile(probes, P, row0, m, N, col0, F, sm, acc);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int cl = wc * 64 + j * 16 + (lane & 15);
            const float rad = col0 + cl < N ? (float)radius[col0 + cl] : -1.0f;      // d >= 0: a column past the end holds nobody
            const float nb = sm.norm[1][cl];
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const float d = pr_dist(sm.norm[0][wr * 64 + i * 16 + (lane >> 4) * 4 + r], nb, acc[i][j][r]);
                    flags |= (d <= rad ? 1u : 0u) << (4 * i + r);
                }
        }
    }
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) flags |= (unsigned)__shfl_xor((int)flags, o, 64);
    if ((lane & 15) == 0) {
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int r = 0; r < 4; r++) sm.list[wc][wr * 64 + i * 16 + (lane >> 4) * 4 + r][0] = (float)((flags >> (4 * i + r)) & 1u);
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (t < PR_T && row0 + t < P) inside[row0 + t] = (sm.list[0][t][0] != 0.f || sm.list[1][t][0] != 0.f) ? 1 : 0;
}

// a feature matrix [n][F] fp16: n > 0, F a positive multiple of 32, rows 16-byte aligned, tile counts within the grid limits
template <typename Kern, typename... Args> void pr_launch(Kern kern, dim3 g, hipStream_t s, Args... args) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(PrSmem));
    hipLaunchKernelGGL(kern, g, dim3(256), sizeof(PrSmem), s, args...);
}

bool pr_ok(const void* x, int n, int F) {
    return x && n > 0 && F > 0 && (F & 31) == 0 && !((uintptr_t)x & 15) && n <= (1 << 24);
}

}  // namespace

extern "C" {

int sidlsg_pr_distances(const void* rows, int R, const void* cols, int C, int F, void* out, void* stream) {
    if (!pr_ok(rows, R, F) || !pr_ok(cols, C, F) || !out || ((uintptr_t)out & 1)) return SIDLSG_EINVAL;
    const dim3 g((unsigned)((C + PR_T - 1) / PR_T), (unsigned)((R + PR_T - 1) / PR_T));
    if (g.y > 65535u) return SIDLSG_EINVAL;
    pr_launch(pr_distances_kernel, g, (hipStream_t)stream, (const f16*)rows, R, (const f16*)cols, C, F, (f16*)out);
    return sidlsg_last_error();
}

int sidlsg_pr_kth_radius(const void* manifold, int N, int F, int k, void* radius_out, void* stream) {
    if (!pr_ok(manifold, N, F) || !radius_out || ((uintptr_t)radius_out & 1) || k < 0 || k >= PR_MAXK1 || N < k + 1) return SIDLSG_EINVAL;
    const dim3 g((unsigned)((N + PR_T - 1) / PR_T));
    hipStream_t s = (hipStream_t)stream;
    const f16* m = (const f16*)manifold;
    f16* ro = (f16*)radius_out;
    if (k < 2) pr_launch(pr_kth_kernel<2>, g, s, m, N, F, k, ro);
    else if (k < 4) pr_launch(pr_kth_kernel<4>, g, s, m, N, F, k, ro);
    else pr_launch(pr_kth_kernel<8>, g, s, m, N, F, k, ro);
    return sidlsg_last_error();
}

int sidlsg_pr_member(const void* probes, int P, const void* manifold, int N, int F, const void* radius, void* inside_out, void* stream) {
    if (!pr_ok(probes, P, F) || !pr_ok(manifold, N, F) || !radius || ((uintptr_t)radius & 1) || !inside_out) return SIDLSG_EINVAL;
    const dim3 g((unsigned)((P + PR_T - 1) / PR_T));
    pr_launch(pr_member_kernel, g, (hipStream_t)stream, (const f16*)probes, P, (const f16*)manifold, N, F,
                       (const f16*)radius, (uint8_t*)inside_out);
    return sidlsg_last_error();
}

}  // extern "C"
