// HPSv2 preprocessing: open_clip's validation transform (Pillow's 8-bit BICUBIC resize of the shorter side, centre crop, ToTensor,
// Normalize) and the patch unfold in one launch (gfx950).  Forward only.
// Compiled with -ffp-contract=off (csrc/build.py EXTRA): the float tail is specified rounding by rounding.
#include "common.h"

// Pillow's ImagingResample for 8-bit channels (src/libImaging/Resample.c) is integer arithmetic once the coefficient bank exists:
// per pass  out = clip8((2^21 + sum_k coeff[k] * in[xmin + k]) >> 22)  with 22-bit fixed-point coefficients, the horizontal pass
// first, the vertical pass on its 8-bit result.  The banks are built on the host in double as Pillow builds them
// (metrics._bicubic_coefficients) and arrive here already restricted to the R x R centre crop:
//   hb [R][2] = (first source column, taps) of cropped output column x, hc [R][hk] its coefficients; vb / vc likewise for rows.
// A side that needs no pass has the bank (x0 + x, 1) / (1 << 22), which the formula above maps to the pixel itself.
constexpr int PIL_BITS = 22;
constexpr int PIL_TABLE_BYTES = 3 * 256 * 4;
constexpr int PIL_LDS_LIMIT = 64 * 1024;

struct PilNorm { float mean[3], std[3]; };

DEVFN int clip8(int v) { return min(max(v, 0), 255); }

// One workgroup per (image, band of P output rows = one row of patches).  The horizontal pass runs over the source rows the band's
// vertical windows touch, for the R cropped columns only, into a uint8 LDS tile [3][band_rows][Rs] (Rs = R rounded up to 4: one
// thread packs 4 columns into one 4-byte LDS store); the vertical pass reads the tile, and the float tail is a 3 x 256-entry table
// ((p / 255 - mean_c) / std_c: an IEEE division, a subtraction, an IEEE division).  In the second phase one thread owns 8
// consecutive columns of one output row, as in clip_patches_kernel: one 16-byte store in bf16, two in fp32, consecutive threads
// consecutive groups.  Every table entry is clamped to the image / the tile before it is used as an index, so a wrong bank gives a
// wrong picture and never an access outside the buffers.
template <typename T>
__global__ __launch_bounds__(256) void pil_patches_kernel(const uint8_t* __restrict__ img, T* __restrict__ out, int H, int W, int R, int P, int Kp,
                                                          const int* __restrict__ hb, const int* __restrict__ hc, int hk,
                                                          const int* __restrict__ vb, const int* __restrict__ vc, int vk, int band_rows,
                                                          PilNorm nrm) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pil_smem[];
    float* tab = reinterpret_cast<float*>(pil_smem);               // [3][256]
    uint8_t* tile = pil_smem + PIL_TABLE_BYTES;                    // [3][band_rows][Rs]
    const int G = R / P, Tn = 1 + G * G, PP = P * P, K = 3 * PP, k8 = Kp >> 3, Rs = (R + 3) & ~3;
    const int b = blockIdx.x / G, band = blockIdx.x - b * G;
    for (int i = threadIdx.x; i < 768; i += 256) {
        const int c = i >> 8;
        const float u = (float)(i & 255) / 255.0f;
        tab[i] = (u - nrm.mean[c]) / nrm.std[c];
    }
    // source rows of the band: the windows move monotonically, so the first row's start and the last row's end bound them all
    const int yl = band * P + P - 1;
    const int y0 = min(max(vb[2 * band * P], 0), H - 1);
    const int nrows = min(max(vb[2 * yl] + vb[2 * yl + 1] - y0, 1), min(band_rows, H - y0));
    const int xq = Rs >> 2;
    for (int i = threadIdx.x; i < 3 * nrows * xq; i += 256) {
        const int q = i % xq, cr = i / xq;
        const int c = cr / nrows, r = cr - c * nrows;
        const uint8_t* line = img + (((size_t)b * 3 + c) * H + (y0 + r)) * W;
        uint32_t pack = 0;
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const int x = q * 4 + e;
            if (x >= R) continue;
            const int x0 = min(max(hb[2 * x], 0), W - 1), n = min(max(hb[2 * x + 1], 0), hk);
            const int* co = hc + (size_t)x * hk;
            int acc = 1 << (PIL_BITS - 1);
            for (int k = 0; k < n; k++) acc += co[k] * (int)line[min(x0 + k, W - 1)];
            pack |= (uint32_t)clip8(acc >> PIL_BITS) << (8 * e);
        }
        *reinterpret_cast<uint32_t*>(tile + ((size_t)c * band_rows + r) * Rs + q * 4) = pack;
    }
    __syncthreads();
    // row b * Tn is the class-token slot (zeros), row b * Tn + 1 + band * G + gx the patch; column k = (c * P + py) * P + px
    for (int i = threadIdx.x; i < G * k8; i += 256) {
        const int gx = i / k8, kq = i - gx * k8;
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const int k = kq * 8 + e;
            v[e] = 0.0f;
            if (k >= K) continue;
            const int c = k / PP, rem = k - c * PP;
            const int py = rem / P, px = rem - py * P;
            const int y = band * P + py, x = gx * P + px;
            const int base = vb[2 * y] - y0, n = min(max(vb[2 * y + 1], 0), vk);
            const int* co = vc + (size_t)y * vk;
            const uint8_t* col = tile + (size_t)c * band_rows * Rs + x;
            int acc = 1 << (PIL_BITS - 1);
            for (int j = 0; j < n; j++) acc += co[j] * (int)col[min(max(base + j, 0), nrows - 1) * Rs];
            v[e] = tab[c * 256 + clip8(acc >> PIL_BITS)];
        }
        stv8<T>(out + ((size_t)b * Tn + 1 + band * G + gx) * Kp + (size_t)kq * 8, v);
    }
    if (band == 0)
        for (int i = threadIdx.x; i < k8; i += 256) zerov8<T>(out + (size_t)b * Tn * Kp + (size_t)i * 8);
}

template <typename T>
static int pil_patches_t(const void* images, void* out, int B, int H, int W, int R, int P, int Kp, const int* hb, const int* hc, int hk,
                         const int* vb, const int* vc, int vk, int band_rows, float m0, float m1, float m2, float s0, float s1, float s2,
                         void* stream) {
    if (!images || !out || !hb || !hc || !vb || !vc || B <= 0 || H <= 0 || W <= 0 || R <= 0 || P <= 0 || R % P) return SIDLSG_EINVAL;
    if ((Kp & 7) || Kp < 3 * P * P || ((uintptr_t)out & 15)) return SIDLSG_EINVAL;
    if ((((uintptr_t)hb | (uintptr_t)hc | (uintptr_t)vb | (uintptr_t)vc) & 3) || hk <= 0 || vk <= 0 || band_rows <= 0) return SIDLSG_EINVAL;
    if (!(s0 != 0.0f) || !(s1 != 0.0f) || !(s2 != 0.0f)) return SIDLSG_EINVAL;
    const long long G = R / P, Tn = 1 + G * G, lim = 1LL << 31, Rs = (R + 3) & ~3;
    if ((long long)B * 3 * H * W >= lim || (long long)B * Tn * Kp >= lim || (long long)B * G >= lim) return SIDLSG_EINVAL;
    const long long lds = PIL_TABLE_BYTES + 3LL * band_rows * Rs;
    if (lds > PIL_LDS_LIMIT) return SIDLSG_EINVAL;
    const PilNorm nrm = {{m0, m1, m2}, {s0, s1, s2}};
    hipLaunchKernelGGL(pil_patches_kernel<T>, dim3((unsigned)(B * G)), dim3(256), (size_t)lds, (hipStream_t)stream, (const uint8_t*)images,
                       (T*)out, H, W, R, P, Kp, hb, hc, hk, vb, vc, vk, band_rows, nrm);
    return sidlsg_last_error();
}

extern "C" {

int sidlsg_pil_patches_u8(const void* images, void* out, int B, int H, int W, int R, int P, int Kp, const int* hbounds, const int* hcoef,
                          int hk, const int* vbounds, const int* vcoef, int vk, int band_rows, float mean0, float mean1, float mean2,
                          float std0, float std1, float std2, void* stream) {
    return pil_patches_t<bf16>(images, out, B, H, W, R, P, Kp, hbounds, hcoef, hk, vbounds, vcoef, vk, band_rows, mean0, mean1, mean2, std0,
                               std1, std2, stream);
}
int sidlsg_pil_patches_u8_f32(const void* images, void* out, int B, int H, int W, int R, int P, int Kp, const int* hbounds, const int* hcoef,
                              int hk, const int* vbounds, const int* vcoef, int vk, int band_rows, float mean0, float mean1, float mean2,
                              float std0, float std1, float std2, void* stream) {
    return pil_patches_t<float>(images, out, B, H, W, R, P, Kp, hbounds, hcoef, hk, vbounds, vcoef, vk, band_rows, mean0, mean1, mean2, std0,
                                std1, std2, stream);
}

}  // extern "C"
