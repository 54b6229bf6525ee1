// LoRA merge on gfx950: every touched layer of a network in ONE launch,
//
//     dst[n][k] = base[n][k] + sum_r coef[r] * up[n][r] * down[r][k]          (all fp32)
//
// on v_mfma_f32_16x16x4_f32 (an exact fp32 fma chain over r, ascending).  Per output element: c_r = coef[r] * up[n][r] rounded once
// while the `up` tile is staged, acc = fma(c_r, down[r][k], acc) for r = 0 .. R - 1 starting from 0, then ONE add of base.  No atomics:
// each element is written once, by the lane that read its base value, so base == dst is allowed and a launch is bit-reproducible.
//
// Geometry.  One workgroup = 256 threads = 4 waves owns a 64 (n) x 64 (k) output tile; wave w owns rows 16 w .. 16 w + 15 as four
// 16 x 16 MFMA tiles along k.  The MFMA computes the TRANSPOSED tile -- A[i][kk] = down[r0 + kk][k0 + i], B[kk][j] = c[n0 + j][r0 + kk]
// -- so lane (j = lane & 15, q = lane >> 4) ends up with out[n0 + j][k0 + 4 q .. 4 q + 3]: four consecutive floats of a master row,
// one 16-byte load of base (issued before the rank loop) and one 16-byte store of dst, 64 contiguous bytes per row and MFMA tile and 256 per
// row over the wave's four.
// Only the factors go through LDS, 32 rank columns at a time: down as [32][64] (row stride 80 floats: the four k-rows of an MFMA step
// fall on disjoint banks), coef * up as [64][32] (row stride 36).  Edges (n >= N, k >= KK, r >= R) are staged as zeros resp. skipped in
// the epilogue; nothing is padded in memory.  KK % 4 == 0 keeps every 16-byte access aligned and entirely inside or outside a row.
#include "common.h"

#define MFMA_F32(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

namespace {

constexpr int LM_T = 64;        // tile edge (n and k)
constexpr int LM_RC = 32;       // rank columns per LDS stage
constexpr int LM_DS = 80;       // row stride of the down image (floats)
constexpr int LM_US = 36;       // row stride of the up image (floats)
constexpr int LM_MAXR = 4096;

struct LmJob { const float* base; float* dst; const float* up; const float* down; const float* coef; int N, KK, R, blk0; };
static_assert(sizeof(LmJob) == 56, "the record layout is part of the C ABI (include/sidlsg_hip.h)");

__global__ __launch_bounds__(256) void lora_merge_kernel(const LmJob* __restrict__ jobs, int njobs) {
    __shared__ __attribute__((aligned(16))) float sD[LM_RC * LM_DS];
    __shared__ __attribute__((aligned(16))) float sU[LM_T * LM_US];
    const int bid = blockIdx.x;
    int lo = 0, hi = njobs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].blk0 <= bid) lo = mid; else hi = mid - 1;
    }
    const LmJob j = jobs[lo];
    const int tk = (j.KK + LM_T - 1) / LM_T;
    const int tile = bid - j.blk0;
    const int n0 = (tile / tk) * LM_T, k0 = (tile % tk) * LM_T;
    if (n0 >= j.N) return;                       // a table that over-counts a job's tiles: nothing to do (block-uniform)
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    f32x4 acc[4];
#pragma unroll
    for (int i = 0; i < 4; i++) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // this lane's 4 x 4 base values, requested before the rank loop; the same lane stores them, which is what makes base == dst safe
    const int n = n0 + wave * 16 + (lane & 15);
    const bool live = n < j.N;
    const size_t row = (size_t)n * j.KK;
    f32x4 v[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int k = k0 + i * 16 + (lane >> 4) * 4;
        v[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (live && k < j.KK) v[i] = *reinterpret_cast<const f32x4*>(j.base + row + k);
    }
    for (int r0 = 0; r0 < j.R; r0 += LM_RC) {
#pragma unroll
        for (int p = 0; p < 2; p++) {
            const int idx = t + 256 * p;
            {   // down[r0 + dr][k0 + 4 c .. + 3], dr 0..31, c 0..15
                const int dr = idx >> 4, c = idx & 15, r = r0 + dr, k = k0 + 4 * c;
                f32x4 d = {0.f, 0.f, 0.f, 0.f};
                if (r < j.R && k < j.KK) d = *reinterpret_cast<const f32x4*>(j.down + (size_t)r * j.KK + k);
                *reinterpret_cast<f32x4*>(sD + dr * LM_DS + 4 * c) = d;
            }
            {   // coef[r] * up[n0 + ur][r0 + 4 c .. + 3], ur 0..63, c 0..7
                const int ur = idx >> 3, c = idx & 7, r = r0 + 4 * c;
                f32x4 cu = {0.f, 0.f, 0.f, 0.f};
                if (n0 + ur < j.N && r < j.R) {
                    const f32x4 u = *reinterpret_cast<const f32x4*>(j.up + (size_t)(n0 + ur) * j.R + r);
                    const f32x4 cf = *reinterpret_cast<const f32x4*>(j.coef + r);
                    cu = (f32x4){__fmul_rn(cf[0], u[0]), __fmul_rn(cf[1], u[1]), __fmul_rn(cf[2], u[2]), __fmul_rn(cf[3], u[3])};
                }
                *reinterpret_cast<f32x4*>(sU + ur * LM_US + 4 * c) = cu;
            }
        }
        __syncthreads();
        const int steps = (j.R - r0 < LM_RC ? j.R - r0 : LM_RC) >> 2;      // R % 4 == 0
        for (int s = 0; s < steps; s++) {
            const int kk = 4 * s + (lane >> 4);
            const float b = sU[(wave * 16 + (lane & 15)) * LM_US + kk];
#pragma unroll
            for (int i = 0; i < 4; i++) acc[i] = MFMA_F32(sD[kk * LM_DS + i * 16 + (lane & 15)], b, acc[i]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int k = k0 + i * 16 + (lane >> 4) * 4;
        if (live && k < j.KK) {
            const f32x4 o = {__fadd_rn(v[i][0], acc[i][0]), __fadd_rn(v[i][1], acc[i][1]), __fadd_rn(v[i][2], acc[i][2]), __fadd_rn(v[i][3], acc[i][3])};
            *reinterpret_cast<f32x4*>(j.dst + row + k) = o;
        }
    }
}

}  // namespace

extern "C" {

int sidlsg_lora_merge_f32(const void* jobs_host, const void* jobs, int njobs, int nblocks, void* stream) {
    if (!jobs_host || !jobs || njobs <= 0 || nblocks <= 0) return SIDLSG_EINVAL;
    const LmJob* h = (const LmJob*)jobs_host;
    long long blk = 0;
    for (int i = 0; i < njobs; i++) {
        const LmJob& j = h[i];
        if (!j.base || !j.dst || !j.up || !j.down || !j.coef) return SIDLSG_EINVAL;
        if ((((uintptr_t)j.base) | ((uintptr_t)j.dst) | ((uintptr_t)j.up) | ((uintptr_t)j.down) | ((uintptr_t)j.coef)) & 15) return SIDLSG_EINVAL;
        if (j.N < 1 || j.KK < 4 || (j.KK & 3) || j.R < 4 || (j.R & 3) || j.R > LM_MAXR) return SIDLSG_EINVAL;
        if ((long long)j.N * j.KK * 4 >= (1ll << 31)) return SIDLSG_EINVAL;
        if (j.blk0 != blk) return SIDLSG_EINVAL;                  // sorted and gap-free: every block maps to exactly one live tile
        blk += (long long)((j.N + LM_T - 1) / LM_T) * ((j.KK + LM_T - 1) / LM_T);
        if (blk > 0x7fffffffll) return SIDLSG_EINVAL;
    }
    if (blk != nblocks) return SIDLSG_EINVAL;
    hipLaunchKernelGGL(lora_merge_kernel, dim3((unsigned)nblocks), dim3(256), 0, (hipStream_t)stream, (const LmJob*)jobs, njobs);
    return sidlsg_last_error();
}

}  // extern "C"
