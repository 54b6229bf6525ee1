// Inpainting: the masked step boundary of the samplers as one launch (gfx950).  Forward only; memory-bound and tiny beside a UNet pass.
#include "common.h"

// ---- masked_renoise -----------------------------------------------------------------------------------------------------------------
// x fp32 NCHW is what a sampler step produced at its target level, z0 fp32 NCHW the scaled init latents, noise fp32 NCHW the initial
// noise z (may be null), mask uint8 [B or 1][HW] (nonzero: repaint), a0 / a1 [B] the coefficients of the target level:
//   known = a0*z0 + a1*noise        rounded a1*noise, then one fma: the expression of noisy_input_kernel, bit-equal to its fp32 x_t
//         = a0*z0                   without noise (one rounded product);  z0 itself without noise and a0.  a0 null means 1.
//   xn    = mask ? x : known        a select, never an interpolation: a NaN on one side does not reach the other
// -> xn fp32 NCHW (may be x itself: every thread reads its elements of x before it writes them) and, when out is not null, the next
// network input NHWC [dup*B][HW][Cp] of T (both halves equal, channels C.. zero), bit-equal to noisy_input(null, xn, 1, 1, dup).
// One thread per (b, pixel) over the C <= 8 channels, as the step kernels.  x and xn may alias, so neither is __restrict__.
template <typename T>
__global__ __launch_bounds__(256) void masked_renoise_kernel(const float* x, const float* __restrict__ z0, const float* __restrict__ noise,
                                                             const unsigned char* __restrict__ mask, const float* __restrict__ a0,
                                                             const float* __restrict__ a1, T* __restrict__ out, float* xn, int B, int C,
                                                             int HW, int Cp, int dup, int mask_shared) {
#pragma clang fp contract(off)
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;  // over B*HW
    if (idx >= B * HW) return;
    const int b = idx / HW, p = idx - b * HW;
    const bool repaint = mask[mask_shared ? (size_t)p : (size_t)idx] != 0;
    const float c0 = a0 ? a0[b] : 1.0f, c1 = noise ? a1[b] : 0.0f;
    float o[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int c = 0; c < 8; c++) {
        if (c >= C) break;
        const size_t i = ((size_t)b * C + c) * HW + p;
        float known = z0[i];
        if (noise) known = __builtin_fmaf(c0, known, c1 * noise[i]);
        else if (a0) known = c0 * known;
        const float v = repaint ? x[i] : known;
        xn[i] = v;
        o[c] = v;
    }
    if (!out) return;
    for (int d = 0; d < dup; d++) {
        T* dst = out + ((size_t)d * B * HW + idx) * Cp;
        stv8<T>(dst, o);
        for (int c = 8; c < Cp; c += 8) zerov8<T>(dst + c);
    }
}

template <typename T>
static int masked_renoise_t(const float* x, const float* z0, const float* noise, const unsigned char* mask, const float* a0,
                            const float* a1, void* out, float* xn, int B, int C, int HW, int Cp, int dup, int mask_shared, void* stream) {
    if (!x || !z0 || !mask || !xn || B < 1 || HW < 1 || C < 1 || C > 8 || Cp % 8 || Cp < 8 || (dup != 1 && dup != 2) ||
        (noise != nullptr) != (a1 != nullptr) || (long long)B * HW > 0x7fffffffLL)
        return SIDLSG_EINVAL;
    const dim3 grid((unsigned)(((size_t)B * HW + 255) / 256));
    hipLaunchKernelGGL(masked_renoise_kernel<T>, grid, dim3(256), 0, (hipStream_t)stream, x, z0, noise, mask, a0, a1, (T*)out, xn, B, C, HW,
                       Cp, dup, mask_shared);
    return sidlsg_last_error();
}

extern "C" {

int sidlsg_masked_renoise(const float* x, const float* z0, const float* noise, const unsigned char* mask, const float* a0,
                          const float* a1, void* out, float* xn, int B, int C, int HW, int Cp, int dup, int mask_shared, void* stream) {
    return masked_renoise_t<bf16>(x, z0, noise, mask, a0, a1, out, xn, B, C, HW, Cp, dup, mask_shared, stream);
}
int sidlsg_masked_renoise_f32(const float* x, const float* z0, const float* noise, const unsigned char* mask, const float* a0,
                              const float* a1, void* out, float* xn, int B, int C, int HW, int Cp, int dup, int mask_shared,
                              void* stream) {
    return masked_renoise_t<float>(x, z0, noise, mask, a0, a1, out, xn, B, C, HW, Cp, dup, mask_shared, stream);
}

}  // extern "C"
