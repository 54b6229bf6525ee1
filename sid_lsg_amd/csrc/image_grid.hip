// Snapshot preview grids (gfx950): decoded fp32 images -> their tiles of one uint8 HWC grid image, on the device.
// Compiled with -ffp-contract=off (csrc/build.py EXTRA): the arithmetic below is specified rounding by rounding.
#include "common.h"

// The arithmetic of the reference's save_image_grid (training/sid_training_loop.py:99-103) in fp32:
//   v = (x - lo) * scale        subtract, then multiply: two roundings, never re-associated or fused
//   v = rint(v)                 to nearest, ties to even (v_rndne_f32), as numpy.rint
//   v = clip(v, 0, 255) -> uint8
// -inf / +inf end as 0 / 255.  NaN is written as 0: numpy's float -> uint8 cast of NaN is undefined, so no fixture pins it.
DEVFN uint32_t grid_u8(float x, float lo, float scale) {
    const float v = rintf(__fmul_rn(__fsub_rn(x, lo), scale));
    return (uint32_t)fminf(fmaxf(v, 0.0f), 255.0f);        // fmaxf first: fmaxf(NaN, 0) = 0
}

// One thread owns 4 consecutive pixels of one image row: 16-byte loads (NHWC8: the first half of each pixel's 8 channels, four
// loads; NCHW: four pixels of a plane, three loads), 12 output bytes as three dwords.  Consecutive threads take consecutive
// pixel groups of a row, so a wave reads and writes contiguous runs.  W % 4 == 0 keeps every access aligned.
template <bool NCHW>
__global__ __launch_bounds__(256) void image_grid_u8_kernel(const float* __restrict__ src, uint8_t* __restrict__ grid, int B, int H,
                                                            int W, int first, int gw, float lo, float scale) {
    const int w4 = W >> 2;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)B * H * w4) return;
    const int xq = (int)(idx % w4);
    const int y = (int)((idx / w4) % H);
    const int b = (int)(idx / ((size_t)w4 * H));
    const int x = xq << 2;
    float4 c[3];     // c[channel] = that channel of the 4 pixels
    if (NCHW) {
        const float* p = src + (((size_t)b * 3) * H + y) * W + x;
        for (int ch = 0; ch < 3; ch++) c[ch] = *(const float4*)(p + (size_t)ch * H * W);
    } else {
        const float* p = src + (((size_t)b * H + y) * W + x) * 8;
        const float4 p0 = *(const float4*)p, p1 = *(const float4*)(p + 8), p2 = *(const float4*)(p + 16), p3 = *(const float4*)(p + 24);
        c[0] = make_float4(p0.x, p1.x, p2.x, p3.x);
        c[1] = make_float4(p0.y, p1.y, p2.y, p3.y);
        c[2] = make_float4(p0.z, p1.z, p2.z, p3.z);
    }
    uint32_t q[12];  // byte 3 * pixel + channel
    for (int ch = 0; ch < 3; ch++) {
        q[0 + ch] = grid_u8(c[ch].x, lo, scale);
        q[3 + ch] = grid_u8(c[ch].y, lo, scale);
        q[6 + ch] = grid_u8(c[ch].z, lo, scale);
        q[9 + ch] = grid_u8(c[ch].w, lo, scale);
    }
    const int tile = first + b;
    const int row = tile / gw, col = tile - row * gw;
    // < 2 GiB by the entry point's check; a multiple of 12 bytes
    const size_t off = (((size_t)row * H + y) * ((size_t)gw * W) + (size_t)col * W + x) * 3;
    uint32_t* dst = (uint32_t*)(grid + off);
    dst[0] = q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24);
    dst[1] = q[4] | (q[5] << 8) | (q[6] << 16) | (q[7] << 24);
    dst[2] = q[8] | (q[9] << 8) | (q[10] << 16) | (q[11] << 24);
}

extern "C" {

int sidlsg_image_grid_u8(const float* src, void* grid, int B, int H, int W, int layout, int first, int gw, int gh, float lo, float hi,
                         void* stream) {
    if (!src || !grid || B <= 0 || H <= 0 || W <= 0 || (W & 3) || gw <= 0 || gh <= 0 || first < 0) return SIDLSG_EINVAL;
    if (layout != 0 && layout != 1) return SIDLSG_EINVAL;
    if ((long long)first + B > (long long)gw * gh) return SIDLSG_EINVAL;
    if (!(hi != lo) || hi != hi || lo != lo) return SIDLSG_EINVAL;
    // the grid fits signed 32-bit byte offsets (and every PNG reader): the four factors are checked one by one against overflow
    const long long lim = 1LL << 31;
    const long long gh_px = (long long)gh * H, gw_px = (long long)gw * W;
    if (gh_px >= lim || gw_px >= lim || gw_px * 3 >= lim || gh_px * (gw_px * 3) >= lim) return SIDLSG_EINVAL;
    if (((uintptr_t)src & 15) || ((uintptr_t)grid & 3)) return SIDLSG_EINVAL;
    // the reference's scale: 255 / (hi - lo) in double, rounded to fp32 where it meets the fp32 image (127.5 for [-1, 1], 1 for [0, 255])
    const float scale = (float)(255.0 / ((double)hi - (double)lo));
    const size_t n = (size_t)B * H * (W >> 2);
    const dim3 g((unsigned)((n + 255) / 256));
    hipStream_t s = (hipStream_t)stream;
    if (layout == 1) hipLaunchKernelGGL(image_grid_u8_kernel<true>, g, dim3(256), 0, s, src, (uint8_t*)grid, B, H, W, first, gw, lo, scale);
    else hipLaunchKernelGGL(image_grid_u8_kernel<false>, g, dim3(256), 0, s, src, (uint8_t*)grid, B, H, W, first, gw, lo, scale);
    return sidlsg_last_error();
}

}  // extern "C"
