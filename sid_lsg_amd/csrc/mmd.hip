// Kernel two-sample statistics (KID: Binkowski et al.; CMMD: Jayasumana et al.) on gfx950: the sums over all pairs of a scalar
// kernel function of the Gram elements of two fp32 feature sets, with the Gram tile never leaving the registers.
//
// Arithmetic (sidlsg_pair_kernel_sums).  g = a . b on v_mfma_f32_16x16x4_f32: an exact fp32 fma chain over k, one rounding per
// product, in the k order of the tile loop below (the same order for every pair and for the norms).
//   kind 0 (polynomial):  v = t * t * t,  t = fma(p0, g, p1)                                  3 fp32 roundings after g
//   kind 1 (RBF):         d2 = max(fma(-2, g, |a|^2 + |b|^2), 0),  v = -expm1f(-(p0 * d2))    = 1 - k: k itself sits within 0.02
//                         of 1 for CMMD, where one fp32 ulp is 6e-8; the complement keeps full relative precision.
// The norms come off the MFMA as in pr_dist.hip (the diagonal of X X^T from the fragments a wave already holds), so a row against
// itself or against a bit-identical duplicate has |a|^2 = |b|^2 = g bit for bit: d2 = 0 and v = 0 exactly.
// Every v is converted to double and summed in double: per lane, by shuffles over the wave, over the 4 waves through LDS, ONE
// double per tile and quantity into `ws`; a second launch adds the slots of a subset in a fixed order.  No atomics, no ticket:
// the same inputs give the same bits on every run.
//
// One workgroup = 256 threads = 4 waves in 2 x 2, a 128 x 128 tile of (rows x columns), 64 x 64 per wave as 4 x 4 MFMA tiles
// (pr_dist.hip's geometry).  Operands are [n][F] fp32 row-major; each is staged global -> registers -> LDS as a [128][32] fp32
// image (128-byte rows, the 16-byte chunk index XORed with row & 7) and read back with one ds_read_b128 per 4 MFMAs: lane
// (r = lane & 15, q = lane >> 4) reads chunk 4 kk + q of its row, and element e of that chunk is its operand of MFMA e, which so
// contracts over k = 16 kk + 4 q + e, q = 0..3.  The k order is permuted against memory order, identically for A, B and the norms.
// Rows are gathered through an index list while staging (16-byte loads); a gathered copy of a subset is never formed.
// Rows past the end of a list and k past F are staged as zeros and MASKED in the epilogue: a zero row has v = p1^3, not 0.
// The symmetric passes (xx, yy) visit only tiles with column tile >= row tile and weight the off-diagonal ones by 2.
#include "common.h"

#define MFMA_F32(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

namespace {

constexpr int MM_T = 128;                  // tile edge (rows and columns)
constexpr int MM_BK = 32;                  // K elements per step
constexpr int MM_IMG = MM_T * MM_BK * 4;   // bytes of one operand image
constexpr int MM_MAXN = 1 << 24, MM_MAXF = 1 << 20;

struct MmSmem {
    unsigned char img[2][2][MM_IMG];       // [buffer][operand: 0 rows, 1 columns]
    float norm[2][MM_T];                   // |.|^2 of the tile's rows / columns (RBF)
    double red[4][2];                      // per wave: sum, diagonal sum
};

DEVFN int mm_off(int row, int chunk) { return row * (MM_BK * 4) + ((chunk ^ (row & 7)) << 4); }

// the 4 chunks this thread stages of one operand: chunk t & 7 of rows (t >> 3) + 32 p of the tile
struct MmStage {
    const float* src[4];       // the row's first element, or null past the end of the list
    u32x4 v[4];
    DEVFN void init(const float* X, int F, const int* idx, int m, int r0, int t) {
#pragma unroll
        for (int p = 0; p < 4; p++) {
            const int li = r0 + (t >> 3) + 32 * p;
            src[p] = nullptr;
            if (li < m) src[p] = X + (size_t)(idx ? idx[li] : li) * F;
        }
    }
    DEVFN void load(int F, int k0, int t) {
        const int k = k0 + ((t & 7) << 2);
#pragma unroll
        for (int p = 0; p < 4; p++) {
            u32x4 q = {0u, 0u, 0u, 0u};
            if (src[p] && k < F) q = *reinterpret_cast<const u32x4*>(src[p] + k);
            v[p] = q;
        }
    }
    DEVFN void store(unsigned char* img, int t) const {
#pragma unroll
        for (int p = 0; p < 4; p++) *reinterpret_cast<u32x4*>(img + mm_off((t >> 3) + 32 * p, t & 7)) = v[p];
    }
};

// acc[i][j][r] = rows[row0 + wr*64 + i*16 + (lane>>4)*4 + r] . cols[col0 + wc*64 + j*16 + (lane&15)];  NORMS: sm.norm = the tile's norms.
// Ends with a barrier: acc and sm.norm are ready, and every wave has left the operand images.
template <bool NORMS>
DEVFN void mm_tile(const float* X, const int* ix, int mr, int row0, const float* Y, const int* iy, int mc, int col0, int F, MmSmem& sm,
                   f32x4 (&acc)[4][4]) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wr = wave >> 1, wc = wave & 1;
    f32x4 na[2], nb[2];      // X X^T blocks of row blocks 2 wc, 2 wc + 1 and column blocks 2 wr, 2 wr + 1 of this wave's quadrant
#pragma unroll
    for (int h = 0; h < 2; h++) na[h] = nb[h] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    MmStage sa, sb;
    sa.init(X, F, ix, mr, row0, t);
    sb.init(Y, F, iy, mc, col0, t);
    const int nk = (F + MM_BK - 1) / MM_BK;
    sa.load(F, 0, t);
    sb.load(F, 0, t);
    sa.store(sm.img[0][0], t);
    sb.store(sm.img[0][1], t);
    __syncthreads();
    for (int s = 0; s < nk; s++) {
        const int cur = s & 1;
        if (s + 1 < nk) {
            sa.load(F, (s + 1) * MM_BK, t);
            sb.load(F, (s + 1) * MM_BK, t);
        }
#pragma unroll
        for (int kk = 0; kk < 2; kk++) {
            f32x4 fa[4], fb[4];
            const int chunk = kk * 4 + (lane >> 4);
#pragma unroll
            for (int i = 0; i < 4; i++) {
                fa[i] = *reinterpret_cast<const f32x4*>(sm.img[cur][0] + mm_off(wr * 64 + i * 16 + (lane & 15), chunk));
                fb[i] = *reinterpret_cast<const f32x4*>(sm.img[cur][1] + mm_off(wc * 64 + i * 16 + (lane & 15), chunk));
            }
#pragma unroll
            for (int e = 0; e < 4; e++) {
#pragma unroll
                for (int i = 0; i < 4; i++)
#pragma unroll
                    for (int j = 0; j < 4; j++) acc[i][j] = MFMA_F32(fa[i][e], fb[j][e], acc[i][j]);
                if constexpr (NORMS) {
#pragma unroll
                    for (int h = 0; h < 2; h++) {
                        const float xa = wc ? fa[2 + h][e] : fa[h][e], xb = wr ? fb[2 + h][e] : fb[h][e];
                        na[h] = MFMA_F32(xa, xa, na[h]);
                        nb[h] = MFMA_F32(xb, xb, nb[h]);
                    }
                }
            }
        }
        if (s + 1 < nk) {
            sa.store(sm.img[cur ^ 1][0], t);
            sb.store(sm.img[cur ^ 1][1], t);
        }
        __syncthreads();
    }
    if constexpr (NORMS) {
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
}

DEVFN double mm_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// first tile of row r of the upper triangle of a T x T tile grid, rows in order, columns r .. T - 1
DEVFN long long mm_tri_off(long long r, long long T) { return r * T - r * (r - 1) / 2; }

struct MmParams {
    const float* X;
    const float* Y;
    const int* ix;
    const int* iy;
    double* ws;
    int F, mx, my, tx, ty, nxx, nyy, ntiles;
    float p0, p1;
};

// grid = (tiles of the three passes, subsets).  Tile ids: [0, nxx) xx upper triangle, [nxx, nxx + nyy) yy, then xy row-major.
// ws[(subset * ntiles + tile) * 2 + {0: weighted sum of v over the tile's live pairs, 1: sum over its i == j pairs (xx, yy)}]
template <int KIND>
__global__ __launch_bounds__(256) void mm_sums_kernel(MmParams p) {
    extern __shared__ __attribute__((aligned(16))) char mm_smem[];
    MmSmem& sm = *reinterpret_cast<MmSmem*>(mm_smem);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wr = wave >> 1, wc = wave & 1;
    const int tile = blockIdx.x, sub = blockIdx.y;
    const float* R = p.X;
    const float* C = p.Y;
    const int* ir = p.ix ? p.ix + (size_t)sub * p.mx : nullptr;
    const int* ic = p.iy ? p.iy + (size_t)sub * p.my : nullptr;
    int mr = p.mx, mc = p.my, rt, ct;
    bool sym = false;
    if (tile < p.nxx + p.nyy) {
        sym = true;
        int q = tile, T = p.tx;
        if (tile < p.nxx) { C = p.X; ic = ir; mc = p.mx; }
        else { q = tile - p.nxx; T = p.ty; R = p.Y; ir = ic; mr = p.my; }
        const double b = 2.0 * T + 1.0;
        int r = (int)((b - sqrt(b * b - 8.0 * q)) * 0.5);
        r = r < 0 ? 0 : r > T - 1 ? T - 1 : r;
        while (r + 1 < T && mm_tri_off(r + 1, T) <= q) r++;
        while (r > 0 && mm_tri_off(r, T) > q) r--;
        rt = r;
        ct = r + (int)(q - mm_tri_off(r, T));
    } else {
        const int q = tile - p.nxx - p.nyy;
        rt = q / p.ty;
        ct = q - rt * p.ty;
    }
    const int row0 = rt * MM_T, col0 = ct * MM_T;
    f32x4 acc[4][4];
    mm_tile<KIND == 1>(R, ir, mr, row0, C, ic, mc, col0, p.F, sm, acc);
    const bool diag = sym && rt == ct;
    double sum = 0.0, dsum = 0.0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int cl = wc * 64 + j * 16 + (lane & 15);
        const bool clive = col0 + cl < mc;
        const float nb = KIND == 1 ? sm.norm[1][cl] : 0.f;
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int rl = wr * 64 + i * 16 + (lane >> 4) * 4 + r;
                const float g = acc[i][j][r];
                float v;
                if constexpr (KIND == 0) {
                    const float tt = __fmaf_rn(p.p0, g, p.p1);
                    v = __fmul_rn(__fmul_rn(tt, tt), tt);
                } else {
                    const float d2 = fmaxf(__fmaf_rn(-2.0f, g, __fadd_rn(sm.norm[0][rl], nb)), 0.0f);
                    v = -expm1f(-__fmul_rn(p.p0, d2));
                }
                const bool live = clive && row0 + rl < mr;      // a padded row or column is a zero vector, not an absent one
                const double dv = live ? (double)v : 0.0;
                sum += dv;
                dsum += (diag && rl == cl) ? dv : 0.0;
            }
    }
    sum = mm_wave_sum(sum);
    dsum = mm_wave_sum(dsum);
    if (lane == 0) { sm.red[wave][0] = sum; sm.red[wave][1] = dsum; }
    __syncthreads();
    if (threadIdx.x < 2) {
        const int k = threadIdx.x;
        const double tot = ((sm.red[0][k] + sm.red[1][k]) + sm.red[2][k]) + sm.red[3][k];
        p.ws[((size_t)sub * p.ntiles + tile) * 2 + k] = (k == 0 && sym && !diag) ? 2.0 * tot : tot;
    }
}

// out[subset][q], q = Sxx, Syy, Sxy, Txx, Tyy: thread t adds slots t, t + 256, .. of the quantity's tile range in that order, then
// the 256 partial sums are added pairwise in a fixed tree.  grid = (5, subsets).
__global__ __launch_bounds__(256) void mm_reduce_kernel(const double* __restrict__ ws, double* __restrict__ out, int nxx, int nyy, int ntiles) {
    __shared__ double part[256];
    const int q = blockIdx.x, sub = blockIdx.y, t = threadIdx.x;
    const int lo = (q == 0 || q == 3) ? 0 : (q == 1 || q == 4) ? nxx : nxx + nyy;
    const int hi = (q == 0 || q == 3) ? nxx : (q == 1 || q == 4) ? nxx + nyy : ntiles;
    const double* w = ws + (size_t)sub * ntiles * 2 + (q >= 3 ? 1 : 0);
    double s = 0.0;
    for (int i = lo + t; i < hi; i += 256) s += w[(size_t)i * 2];
    part[t] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) part[t] += part[t + o];
        __syncthreads();
    }
    if (t == 0) out[sub * 5 + q] = part[0];
}

// tile counts of one subset; false when a count or the workspace does not fit the int arithmetic of the kernels
bool mm_geometry(int S, int mx, int my, int* tx, int* ty, int* nxx, int* nyy, int* ntiles) {
    if (S < 1 || S > 65535 || mx < 1 || my < 1 || mx > MM_MAXN || my > MM_MAXN) return false;
    const long long a = (mx + MM_T - 1) / MM_T, b = (my + MM_T - 1) / MM_T;
    const long long xx = a * (a + 1) / 2, yy = b * (b + 1) / 2, all = xx + yy + a * b;
    if (all * 2 * S > 0x7FFFFFFFll) return false;
    *tx = (int)a; *ty = (int)b; *nxx = (int)xx; *nyy = (int)yy; *ntiles = (int)all;
    return true;
}

}  // namespace

extern "C" {

int sidlsg_pair_kernel_sums_ws_doubles(int S, int mx, int my) {
    int tx, ty, nxx, nyy, ntiles;
    if (!mm_geometry(S, mx, my, &tx, &ty, &nxx, &nyy, &ntiles)) return -1;
    return 2 * S * ntiles;
}

int sidlsg_pair_kernel_sums(const float* X, int nx, const float* Y, int ny, int F, const int* ix, const int* iy, int S, int mx, int my,
                            int kind, float p0, float p1, double* out, double* ws, void* stream) {
    MmParams p;
    if (!X || !Y || !out || !ws || ((uintptr_t)X & 15) || ((uintptr_t)Y & 15) || ((uintptr_t)out & 7) || ((uintptr_t)ws & 7)) return SIDLSG_EINVAL;
    if (nx < 1 || ny < 1 || nx > MM_MAXN || ny > MM_MAXN || F < 4 || (F & 3) || F > MM_MAXF || kind < 0 || kind > 1) return SIDLSG_EINVAL;
    if ((ix == nullptr) != (iy == nullptr) || ((uintptr_t)ix & 3) || ((uintptr_t)iy & 3)) return SIDLSG_EINVAL;
    if (!ix && (S != 1 || mx != nx || my != ny)) return SIDLSG_EINVAL;
    if (!mm_geometry(S, mx, my, &p.tx, &p.ty, &p.nxx, &p.nyy, &p.ntiles)) return SIDLSG_EINVAL;
    p.X = X; p.Y = Y; p.ix = ix; p.iy = iy; p.ws = ws; p.F = F; p.mx = mx; p.my = my; p.p0 = p0; p.p1 = p1;
    hipStream_t s = (hipStream_t)stream;
    const dim3 g((unsigned)p.ntiles, (unsigned)S);
    if (kind == 0) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(mm_sums_kernel<0>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(MmSmem));
        hipLaunchKernelGGL(mm_sums_kernel<0>, g, dim3(256), sizeof(MmSmem), s, p);
    } else {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(mm_sums_kernel<1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(MmSmem));
        hipLaunchKernelGGL(mm_sums_kernel<1>, g, dim3(256), sizeof(MmSmem), s, p);
    }
    hipLaunchKernelGGL(mm_reduce_kernel, dim3(5, (unsigned)S), dim3(256), 0, s, (const double*)ws, out, p.nxx, p.nyy, p.ntiles);
    return sidlsg_last_error();
}

}  // extern "C"
