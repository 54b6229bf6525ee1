// The two ends of AutoencoderKL.encode around the encoder's convolutions (gfx950): images -> the conv_in activation layout, and the
// moments -> the scaled latent sample.  Compiled with -ffp-contract=off (csrc/build.py EXTRA): both are specified rounding by rounding.
#include "common.h"
#include <math.h>

namespace {

// [B][H][W][3] uint8 -> [B][H][W][8] bf16: x / 127.5 - 1 (an IEEE fp32 division, then a subtraction: the value numpy and torch form on the
// host from the same expression), rounded to nearest even; channels 3..7 zero.  One thread per pixel: 3 byte loads, one 16-byte store.
__global__ __launch_bounds__(256) void image_u8_to_nhwc8_kernel(const uint8_t* __restrict__ src, bf16* __restrict__ dst, size_t npix) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= npix) return;
    const uint8_t* s = src + i * 3;
    bf16x8 o = zero8();
#pragma unroll
    for (int c = 0; c < 3; c++) o[c] = f2bf(__fsub_rn(__fdiv_rn((float)s[c], 127.5f), 1.0f));
    st8(dst + i * 8, o);
}

// [B][3][H][W] fp32 (already in [-1, 1]) -> the same layout: a rounding to bf16 and the NCHW -> NHWC move
__global__ __launch_bounds__(256) void image_f32_to_nhwc8_kernel(const float* __restrict__ src, bf16* __restrict__ dst, int B, size_t hw) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)B * hw) return;
    const size_t b = i / hw, px = i - b * hw;
    const float* s = src + b * 3 * hw + px;
    bf16x8 o = zero8();
#pragma unroll
    for (int c = 0; c < 3; c++) o[c] = f2bf(s[c * hw]);
    st8(dst + i * 8, o);
}

// moments [B][HW][8] fp32 (the encoder's conv_out, NHWC) -> quant_conv (8 x 8 + bias per pixel), DiagonalGaussianDistribution
// (diffusers: mean, logvar = chunk(2); logvar.clamp(-30, 20); std = exp(0.5 logvar)), z = (mean + std * eps) * scaling, fp32 NCHW.
// One thread per pixel; consecutive threads take consecutive pixels of a plane, so every NCHW access is contiguous per channel.
__global__ __launch_bounds__(256) void vae_posterior_kernel(const float* __restrict__ mom, const float* __restrict__ qw, const float* __restrict__ qb,
                                                            const float* __restrict__ eps, float* __restrict__ z, float* __restrict__ mean,
                                                            float* __restrict__ logvar, int B, size_t hw, float scaling) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)B * hw) return;
    const size_t b = i / hw, px = i - b * hw;
    const f32x4 y0 = *reinterpret_cast<const f32x4*>(mom + i * 8), y1 = *reinterpret_cast<const f32x4*>(mom + i * 8 + 4);
    const float y[8] = {y0[0], y0[1], y0[2], y0[3], y1[0], y1[1], y1[2], y1[3]};
    float o[8];
#pragma unroll
    for (int n = 0; n < 8; n++) {
        float a = qb[n];
#pragma unroll
        for (int k = 0; k < 8; k++) a = fmaf(qw[n * 8 + k], y[k], a);
        o[n] = a;
    }
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const size_t at = (b * 4 + c) * hw + px;
        const float lv = fminf(fmaxf(o[4 + c], -30.0f), 20.0f);
        float v = o[c];
        if (eps) v = v + expf(0.5f * lv) * eps[at];
        z[at] = v * scaling;
        if (mean) mean[at] = o[c];
        if (logvar) logvar[at] = lv;
    }
}

}  // namespace

extern "C" {

int sidlsg_image_to_nhwc8(const void* images_u8, void* out, int B, int H, int W, void* stream) {
    if (!images_u8 || !out || B <= 0 || H <= 0 || W <= 0 || ((uintptr_t)out & 15)) return SIDLSG_EINVAL;
    const size_t npix = (size_t)B * H * W;
    if (npix >= (1ull << 31)) return SIDLSG_EINVAL;
    hipLaunchKernelGGL(image_u8_to_nhwc8_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)images_u8,
                       (bf16*)out, npix);
    return sidlsg_last_error();
}

int sidlsg_image_to_nhwc8_f32(const float* images_nchw, void* out, int B, int H, int W, void* stream) {
    if (!images_nchw || !out || B <= 0 || H <= 0 || W <= 0 || ((uintptr_t)out & 15)) return SIDLSG_EINVAL;
    const size_t hw = (size_t)H * W;
    if ((size_t)B * hw >= (1ull << 31)) return SIDLSG_EINVAL;
    hipLaunchKernelGGL(image_f32_to_nhwc8_kernel, dim3((unsigned)(((size_t)B * hw + 255) / 256)), dim3(256), 0, (hipStream_t)stream, images_nchw,
                       (bf16*)out, B, hw);
    return sidlsg_last_error();
}

int sidlsg_vae_posterior(const float* moments, const float* qw, const float* qb, const float* eps, float* z, float* mean, float* logvar, int B,
                         int HW, float scaling, void* stream) {
    if (!moments || !qw || !qb || !z || B <= 0 || HW <= 0 || ((uintptr_t)moments & 15)) return SIDLSG_EINVAL;
    const size_t n = (size_t)B * HW;
    if (n >= (1ull << 31)) return SIDLSG_EINVAL;
    hipLaunchKernelGGL(vae_posterior_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, moments, qw, qb, eps, z, mean, logvar,
                       B, (size_t)HW, scaling);
    return sidlsg_last_error();
}

}  // extern "C"
