// ControlNet: the control images -> the hint embedder's input (gfx950).  Everything else a ControlNet computes runs on the UNet's GEMM /
// conv / norm / attention entry points.  Compiled with -ffp-contract=off (csrc/build.py EXTRA) like the other image conversions: the value
// is specified as one IEEE fp32 division (then, for bf16, one rounding to nearest even).
#include "common.h"

namespace {

// [B][H][W][3] uint8 -> [B][H][W][8] bf16 / fp32: float(x) / 255; channels 3..7 zero.  One thread per pixel: 3 byte loads, one 16-byte
// (bf16) or two 16-byte (fp32) stores.
template <typename T>
__global__ __launch_bounds__(256) void control_hint_u8_kernel(const uint8_t* __restrict__ src, T* __restrict__ dst, size_t npix) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= npix) return;
    const uint8_t* s = src + i * 3;
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; c++) v[c] = __fdiv_rn((float)s[c], 255.0f);
    if constexpr (sizeof(T) == 2) {
        bf16x8 o = zero8();
#pragma unroll
        for (int c = 0; c < 3; c++) o[c] = f2bf(v[c]);
        st8(dst + i * 8, o);
    } else {
        f32x4 lo = {v[0], v[1], v[2], 0.0f}, hi = {0.0f, 0.0f, 0.0f, 0.0f};
        *reinterpret_cast<f32x4*>(dst + i * 8) = lo;
        *reinterpret_cast<f32x4*>(dst + i * 8 + 4) = hi;
    }
}

}  // namespace

extern "C" {

int sidlsg_control_hint_u8(const void* images_u8, void* out, int B, int H, int W, int f32_out, void* stream) {
    if (!images_u8 || !out || B <= 0 || H <= 0 || W <= 0 || ((uintptr_t)out & 15)) return SIDLSG_EINVAL;
    const size_t npix = (size_t)B * H * W;
    if (npix * 8 * (f32_out ? 4 : 2) >= (1ull << 31)) return SIDLSG_EINVAL;
    const dim3 grid((unsigned)((npix + 255) / 256));
    if (f32_out)
        hipLaunchKernelGGL(control_hint_u8_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const uint8_t*)images_u8, (float*)out, npix);
    else
        hipLaunchKernelGGL(control_hint_u8_kernel<bf16>, grid, dim3(256), 0, (hipStream_t)stream, (const uint8_t*)images_u8, (bf16*)out, npix);
    return sidlsg_last_error();
}

}  // extern "C"
