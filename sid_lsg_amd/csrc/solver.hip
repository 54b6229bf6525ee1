// Teacher sampler: one step boundary of a solver family (DDIM with any eta, DPM-Solver++ 2M) as one launch, and the per-sample
// statistics of the guidance rescale (Lin et al. 2024) (gfx950).  Forward only; memory-bound and tiny beside a UNet pass.
#include "common.h"

// ---- solver_step --------------------------------------------------------------------------------------------------------------------
// eps [dup*B][HW][Ce] fp32 is the teacher's output at s ([uncond ; cond] when dup = 2), xt fp32 NCHW is x_s, s0/s1 [B] are
// alpha_s / sigma_s, coef [B][4] = (c_x, c_cur, c_prev, c_n) of scheduler.solver_schedule:
//   e  = dup == 2 ? u + kappa*(c - u) : eps                           cfg_x0_kernel<0>
//   e  = e*scale[b]                     (scale may be null)           the guidance rescale, one rounded product
//   x0 = (x_s - s1*e)/s0 (MODE 1) | s0*x_s - s1*e (MODE 2)            cfg_x0_kernel<MODE>
//   x_t = c_x*x_s + c_cur*x0 + c_prev*x0p + c_n*noise                 a rounded product, then one fma per term in this order
// x0p (the x0 prediction of the step before) and noise are fp32 NCHW and may be null: their term is then not formed, which gives the
// bits of a zero tensor with a zero coefficient.
// -> out NHWC [dup*B][HW][Cp] of T (both halves equal, channels C.. zero; may be null), xtn fp32 NCHW, x0 fp32 NCHW (may be null).
// The roundings are spelled out (contraction is off in the body) as in ddim_step_kernel, so with scale null x0 is bit-equal to
// cfg_x0<MODE>.  VEC: Ce == 8 and eps 16-byte aligned (the network's output), else element loads as cfg_x0_kernel.
template <typename T, int MODE, bool VEC>
__global__ __launch_bounds__(256) void solver_step_kernel(const float* __restrict__ eps, const float* __restrict__ xt,
                                                          const float* __restrict__ s0, const float* __restrict__ s1,
                                                          const float* __restrict__ coef, const float* __restrict__ x0p,
                                                          const float* __restrict__ noise, const float* __restrict__ scale,
                                                          T* __restrict__ out, float* __restrict__ xtn, float* __restrict__ x0,
                                                          int B, int C, int HW, int Ce, int Cp, int dup, float kappa) {
#pragma clang fp contract(off)
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;  // over B*HW
    if (idx >= B * HW) return;
    const int b = idx / HW, p = idx - b * HW;
    const float* eu = eps + (size_t)idx * Ce;
    const float* ec = eps + ((size_t)B * HW + idx) * Ce;
    float u[8] = {0, 0, 0, 0, 0, 0, 0, 0}, cn[8] = {0, 0, 0, 0, 0, 0, 0, 0}, o[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (VEC) {
        ldv8<float>(eu, u);
        if (dup == 2) ldv8<float>(ec, cn);
    } else {
        for (int c = 0; c < C; c++) { u[c] = eu[c]; if (dup == 2) cn[c] = ec[c]; }
    }
    const float a0 = s0[b], a1 = s1[b];
    const float cx = coef[4 * b], cc = coef[4 * b + 1], cp = coef[4 * b + 2], cz = coef[4 * b + 3];
    const float sc = scale ? scale[b] : 1.0f;
#pragma unroll
    for (int c = 0; c < 8; c++) {
        if (c >= C) break;
        const size_t i = ((size_t)b * C + c) * HW + p;
        const float x = xt[i];
        float e = dup == 2 ? __builtin_fmaf(kappa, cn[c] - u[c], u[c]) : u[c];
        if (scale) e = e * sc;
        const float xh = MODE == 1 ? __builtin_fmaf(-a1, e, x) / a0 : a0 * x - a1 * e;
        float v = __builtin_fmaf(cc, xh, cx * x);
        if (x0p) v = __builtin_fmaf(cp, x0p[i], v);
        if (noise) v = __builtin_fmaf(cz, noise[i], v);
        xtn[i] = v;
        if (x0) x0[i] = xh;
        o[c] = v;
    }
    if (!out) return;
    for (int d = 0; d < dup; d++) {
        T* dst = out + ((size_t)d * B * HW + idx) * Cp;
        stv8<T>(dst, o);
        for (int c = 8; c < Cp; c += 8) zerov8<T>(dst + c);
    }
}

// ---- cfg_rescale_stats ----------------------------------------------------------------------------------------------------------------
// scale[b] = phi*std(c_b)/std(g_b) + 1 - phi with g = u + kappa*(c - u) (the fma of solver_step_kernel), the standard deviations over
// the C*HW real channels of sample b, unbiased (n - 1): diffusers' rescale_noise_cfg as one factor per sample.  std(g_b) = 0 gives 1
// (diffusers divides and yields NaN).  One workgroup per sample; two passes over the sample's 2*C*HW values (a few tens of KB, the
// second pass reads them from the cache): the means, then the squared distances from them -- never E[x^2] - E[x]^2.  The order of
// every sum is fixed: a thread adds its positions in ascending order, the 64 lanes of a wave combine in a butterfly, the four wave
// partials are added in wave order by every thread.  No atomics.  A NaN stays in its sample's factor.
DEVFN float stats_block_sum(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();                       // the previous use of red[] is over
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

template <bool VEC>
__global__ __launch_bounds__(256) void cfg_rescale_stats_kernel(const float* __restrict__ eps, float* __restrict__ scale, int B, int C,
                                                                int HW, int Ce, float kappa, float phi) {
#pragma clang fp contract(off)
    __shared__ float red[4];
    const int b = blockIdx.x;
    const float* eu = eps + (size_t)b * HW * Ce;
    const float* ec = eps + ((size_t)B + b) * HW * Ce;
    const float n = (float)C * (float)HW;
    float mean_g = 0.0f, mean_c = 0.0f, var_g = 0.0f, var_c = 0.0f;
    for (int pass = 0; pass < 2; pass++) {
        float sg = 0.0f, sc = 0.0f;
        for (int p = threadIdx.x; p < HW; p += 256) {
            float u[8] = {0, 0, 0, 0, 0, 0, 0, 0}, cn[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            if (VEC) {
                ldv8<float>(eu + (size_t)p * Ce, u);
                ldv8<float>(ec + (size_t)p * Ce, cn);
            } else {
                for (int c = 0; c < C; c++) { u[c] = eu[(size_t)p * Ce + c]; cn[c] = ec[(size_t)p * Ce + c]; }
            }
#pragma unroll
            for (int c = 0; c < 8; c++) {
                if (c >= C) break;
                const float g = __builtin_fmaf(kappa, cn[c] - u[c], u[c]);
                if (pass == 0) { sg += g; sc += cn[c]; }
                else { const float dg = g - mean_g, dc = cn[c] - mean_c; sg = __builtin_fmaf(dg, dg, sg); sc = __builtin_fmaf(dc, dc, sc); }
            }
        }
        sg = stats_block_sum(sg, red);
        sc = stats_block_sum(sc, red);
        if (pass == 0) { mean_g = sg / n; mean_c = sc / n; }
        else { var_g = sg / (n - 1.0f); var_c = sc / (n - 1.0f); }
    }
    if (threadIdx.x == 0) {
        const float sd_g = sqrtf(var_g), sd_c = sqrtf(var_c);
        scale[b] = sd_g == 0.0f ? 1.0f : __builtin_fmaf(phi, sd_c / sd_g, 1.0f - phi);
    }
}

template <typename T>
static int solver_step_t(const float* eps, const float* xt, const float* s0, const float* s1, const float* coef, const float* x0p,
                         const float* noise, const float* scale, void* out, float* xtn, float* x0, int B, int C, int HW, int Ce, int Cp,
                         int dup, float kappa, int mode, int need_prev, void* stream) {
    if (!eps || !xt || !s0 || !s1 || !coef || !xtn || B < 1 || HW < 1 || C < 1 || C > 8 || Ce < C || Cp % 8 || Cp < 8 ||
        (dup != 1 && dup != 2) || (mode != 1 && mode != 2) || (long long)B * HW > 0x7fffffffLL || (need_prev && !x0p))
        return SIDLSG_EINVAL;
    const dim3 grid((unsigned)(((size_t)B * HW + 255) / 256));
    hipStream_t s = (hipStream_t)stream;
    const bool vec = Ce == 8 && (((uintptr_t)eps) & 15) == 0;
#define SIDLSG_SOLVER(M, V) hipLaunchKernelGGL((solver_step_kernel<T, M, V>), grid, dim3(256), 0, s, eps, xt, s0, s1, coef, x0p, noise, scale, (T*)out, xtn, x0, B, C, HW, Ce, Cp, dup, kappa)
    if (mode == 1) { if (vec) SIDLSG_SOLVER(1, true); else SIDLSG_SOLVER(1, false); }
    else { if (vec) SIDLSG_SOLVER(2, true); else SIDLSG_SOLVER(2, false); }
#undef SIDLSG_SOLVER
    return sidlsg_last_error();
}

extern "C" {

int sidlsg_solver_step(const float* eps, const float* xt, const float* s0, const float* s1, const float* coef, const float* x0p,
                       const float* noise, const float* scale, void* out, float* xtn, float* x0, int B, int C, int HW, int Ce, int Cp,
                       int dup, float kappa, int mode, int need_prev, void* stream) {
    return solver_step_t<bf16>(eps, xt, s0, s1, coef, x0p, noise, scale, out, xtn, x0, B, C, HW, Ce, Cp, dup, kappa, mode, need_prev, stream);
}
int sidlsg_solver_step_f32(const float* eps, const float* xt, const float* s0, const float* s1, const float* coef, const float* x0p,
                           const float* noise, const float* scale, void* out, float* xtn, float* x0, int B, int C, int HW, int Ce, int Cp,
                           int dup, float kappa, int mode, int need_prev, void* stream) {
    return solver_step_t<float>(eps, xt, s0, s1, coef, x0p, noise, scale, out, xtn, x0, B, C, HW, Ce, Cp, dup, kappa, mode, need_prev, stream);
}

int sidlsg_cfg_rescale_stats(const float* eps, float* scale, int B, int C, int HW, int Ce, float kappa, float phi, void* stream) {
    if (!eps || !scale || B < 1 || HW < 1 || C < 1 || C > 8 || Ce < C || (long long)C * HW < 2 || (long long)2 * B * HW * Ce > 0x7fffffffLL)
        return SIDLSG_EINVAL;
    const bool vec = Ce == 8 && (((uintptr_t)eps) & 15) == 0;
    if (vec) hipLaunchKernelGGL(cfg_rescale_stats_kernel<true>, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, eps, scale, B, C, HW, Ce, kappa, phi);
    else hipLaunchKernelGGL(cfg_rescale_stats_kernel<false>, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, eps, scale, B, C, HW, Ce, kappa, phi);
    return sidlsg_last_error();
}

}  // extern "C"
