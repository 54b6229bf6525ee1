// CLIP image tower, the three kernels the ViT needs beside GEMM / LayerNorm / attention (gfx950).  Forward only.
// Compiled with -ffp-contract=off (csrc/build.py EXTRA): the resampling below is specified rounding by rounding.
#include "common.h"

// ---- preprocessing: uint8 NCHW -> the A operand of the patch-embedding GEMM ---------------------------------------------------
// The reference wrapper's lines (networks/clip.py:33-37) in fp32:
//   v = x / 255                                                         one IEEE division per source pixel (a 256-entry table)
//   v = F.interpolate(v, R, mode='bicubic', align_corners=False)        A = -0.75, src = (dst + 0.5) * in / out - 0.5, taps clamped
//   v = (v - mean_c) / std_c                                            to the border, no antialiasing, overshoot kept
// Weights of the four taps around src = floor + t (aten UpSampleKernel: cubic_convolution1 / 2, Horner form):
DEVFN float cubic_in(float x, float A) { return ((A + 2.0f) * x - (A + 3.0f)) * x * x + 1.0f; }        // |x| <= 1
DEVFN float cubic_out(float x, float A) { return ((A * x - 5.0f * A) * x + 8.0f * A) * x - 4.0f * A; }  // 1 < |x| < 2
DEVFN void cubic_taps(int dst, float scale, int in, int (&idx)[4], float (&w)[4]) {
    const float A = -0.75f;
    const float src = scale * ((float)dst + 0.5f) - 0.5f;
    const float fl = floorf(src);
    const float t = src - fl;
    const int i0 = (int)fl;
    w[0] = cubic_out(t + 1.0f, A);
    w[1] = cubic_in(t, A);
    w[2] = cubic_in(1.0f - t, A);
    w[3] = cubic_out(2.0f - t, A);
#pragma unroll
    for (int k = 0; k < 4; k++) idx[k] = min(max(i0 - 1 + k, 0), in - 1);
}

struct ClipNorm { float mean[3], std[3]; };

// One thread owns 8 consecutive columns of one output row (one 16-byte store in bf16, two in fp32); consecutive threads take
// consecutive column groups, so a wave writes one contiguous run.  Row r = b * T + t: t = 0 is the class-token slot (zeros; the
// class embedding arrives through the GEMM's res operand), t - 1 = gy * G + gx the patch.  Column k = (c * P + py) * P + px, the
// order of the flattened patch_embedding.weight; columns K .. Kp - 1 are zero padding.
template <typename T>
__global__ __launch_bounds__(256) void clip_patches_kernel(const uint8_t* __restrict__ img, T* __restrict__ out, int B, int H, int W, int R,
                                                           int P, int Kp, ClipNorm nrm, float sy, float sx) {
    __shared__ float unit[256];
    unit[threadIdx.x] = (float)threadIdx.x / 255.0f;
    __syncthreads();
    const int G = R / P, Tn = 1 + G * G, K = 3 * P * P, k8 = Kp >> 3;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)B * Tn * k8) return;
    const int kq = (int)(idx % k8);
    const size_t row = idx / k8;
    const int t = (int)(row % Tn);
    const int b = (int)(row / Tn);
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; e++) {
        const int k = kq * 8 + e;
        v[e] = 0.0f;
        if (t == 0 || k >= K) continue;
        const int c = k / (P * P), rem = k - c * P * P;
        const int py = rem / P, px = rem - py * P;
        const int gy = (t - 1) / G, gx = (t - 1) - gy * G;
        int iy[4], ix[4];
        float wy[4], wx[4];
        cubic_taps(gy * P + py, sy, H, iy, wy);
        cubic_taps(gx * P + px, sx, W, ix, wx);
        const uint8_t* plane = img + ((size_t)b * 3 + c) * H * W;
        float acc = 0.0f;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint8_t* line = plane + (size_t)iy[j] * W;
            const float h = unit[line[ix[0]]] * wx[0] + unit[line[ix[1]]] * wx[1] + unit[line[ix[2]]] * wx[2] + unit[line[ix[3]]] * wx[3];
            acc = acc + h * wy[j];
        }
        v[e] = (acc - nrm.mean[c]) / nrm.std[c];
    }
    stv8<T>(out + row * Kp + (size_t)kq * 8, v);
}

// ---- GELU of the MLP (the bias stays in the fc1 GEMM's epilogue) ---------------------------------------------------------------
// mode 0: quick_gelu x * sigmoid(1.702 x) (OpenAI checkpoints) as x / (1 + exp(-1.702 x)).
// mode 1: the exact GELU x * Phi(x) (open_clip ViT-H / ViT-g) as 0.5 x erfc(-x / sqrt 2): erfc keeps its relative accuracy in the
// negative tail, where 1 + erf(x / sqrt 2) cancels to nothing.  Both dtypes evaluate in fp32; bf16 rounds once at the store.
template <int MODE> DEVFN float clip_gelu(float x) {
    if (MODE == 0) return x / (1.0f + expf(-1.702f * x));
    return 0.5f * x * erfcf(-0.70710678118654752f * x);
}
template <typename T, int MODE>
__global__ __launch_bounds__(256) void clip_gelu_kernel(const T* __restrict__ x, T* __restrict__ y, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long n8 = n >> 3;
    if (i < n8) {
        float v[8];
        ldv8<T>(x + i * 8, v);
#pragma unroll
        for (int e = 0; e < 8; e++) v[e] = clip_gelu<MODE>(v[e]);
        stv8<T>(y + i * 8, v);
    } else if (i == n8) {                          // the n % 8 elements behind the last full group
        for (long long j = n8 * 8; j < n; j++) y[j] = (T)clip_gelu<MODE>((float)x[j]);
    }
}

// ---- CLIP score: F.normalize of both embeddings and the row cosine -----------------------------------------------------------
// One wave per row.  V elements per lane and step: 4 (16-byte fp32 loads and stores, 8-byte bf16 loads) when F % 4 == 0, else 1.
template <typename T, int V> DEVFN void ld_row(const T* p, float (&v)[V]) {
    if constexpr (V == 1) {
        v[0] = (float)p[0];
    } else if constexpr (sizeof(T) == 4) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(p);
        v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3];
    } else {
        const bf16x4 a = *reinterpret_cast<const bf16x4*>(p);
        v[0] = bf2f(a[0]); v[1] = bf2f(a[1]); v[2] = bf2f(a[2]); v[3] = bf2f(a[3]);
    }
}
template <typename T, int V>
__global__ __launch_bounds__(256) void clip_score_kernel(const T* __restrict__ img, const T* __restrict__ txt, float* __restrict__ feats,
                                                         float* __restrict__ cosine, int B, int F, float eps) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= B) return;                          // whole waves leave together
    const T* a = img + (size_t)row * F;
    const T* t = txt + (size_t)row * F;
    float sa = 0.0f, st = 0.0f;
    for (int i = lane * V; i < F; i += 64 * V) {
        float va[V], vt[V];
        ld_row<T, V>(a + i, va);
        ld_row<T, V>(t + i, vt);
#pragma unroll
        for (int e = 0; e < V; e++) { sa += va[e] * va[e]; st += vt[e] * vt[e]; }
    }
    const float na = fmaxf(sqrtf(wave_sum(sa)), eps), nt = fmaxf(sqrtf(wave_sum(st)), eps);    // F.normalize: x / max(|x|, eps)
    float* o = feats + (size_t)row * 2 * F;
    float dot = 0.0f;
    for (int i = lane * V; i < F; i += 64 * V) {
        float va[V], vt[V];
        ld_row<T, V>(a + i, va);
        ld_row<T, V>(t + i, vt);
#pragma unroll
        for (int e = 0; e < V; e++) { va[e] = va[e] / na; vt[e] = vt[e] / nt; dot += va[e] * vt[e]; }
        if constexpr (V == 4) {
            *reinterpret_cast<f32x4*>(o + i) = (f32x4){va[0], va[1], va[2], va[3]};
            *reinterpret_cast<f32x4*>(o + F + i) = (f32x4){vt[0], vt[1], vt[2], vt[3]};
        } else {
            o[i] = va[0];
            o[F + i] = vt[0];
        }
    }
    dot = wave_sum(dot);
    if (lane == 0) cosine[row] = dot;
}

template <typename T>
static int clip_patches_t(const void* images, void* out, int B, int H, int W, int R, int P, int Kp, float m0, float m1, float m2,
                          float s0, float s1, float s2, void* stream) {
    if (!images || !out || B <= 0 || H <= 0 || W <= 0 || R <= 0 || P <= 0 || R % P) return SIDLSG_EINVAL;
    if ((Kp & 7) || Kp < 3 * P * P || ((uintptr_t)out & 15)) return SIDLSG_EINVAL;
    if (!(s0 != 0.0f) || !(s1 != 0.0f) || !(s2 != 0.0f)) return SIDLSG_EINVAL;
    const long long G = R / P, Tn = 1 + G * G, lim = 1LL << 31;
    if ((long long)B * 3 * H * W >= lim || (long long)B * Tn * Kp >= lim) return SIDLSG_EINVAL;
    const ClipNorm nrm = {{m0, m1, m2}, {s0, s1, s2}};
    // aten's area_pixel_compute_scale: the ratio formed in fp32
    const float sy = (float)H / (float)R, sx = (float)W / (float)R;
    const size_t n = (size_t)B * Tn * (Kp >> 3);
    hipLaunchKernelGGL(clip_patches_kernel<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)images,
                       (T*)out, B, H, W, R, P, Kp, nrm, sy, sx);
    return sidlsg_last_error();
}

template <typename T>
static int clip_gelu_t(const void* x, void* y, long long n, int mode, void* stream) {
    if (!x || !y || n <= 0 || (mode != 0 && mode != 1) || (((uintptr_t)x | (uintptr_t)y) & 15)) return SIDLSG_EINVAL;
    const long long threads = (n >> 3) + 1, blocks = (threads + 255) / 256;
    if (blocks >= (1LL << 31)) return SIDLSG_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (mode == 0) hipLaunchKernelGGL((clip_gelu_kernel<T, 0>), dim3((unsigned)blocks), dim3(256), 0, s, (const T*)x, (T*)y, n);
    else hipLaunchKernelGGL((clip_gelu_kernel<T, 1>), dim3((unsigned)blocks), dim3(256), 0, s, (const T*)x, (T*)y, n);
    return sidlsg_last_error();
}

template <typename T>
static int clip_score_t(const void* img, const void* txt, float* feats, float* cosine, int B, int F, void* stream) {
    const dim3 g((unsigned)((B + 3) / 4));
    hipStream_t s = (hipStream_t)stream;
    const float eps = 1e-12f;
    const bool vec = !(F & 3) && !(((uintptr_t)img | (uintptr_t)txt) & (4 * sizeof(T) - 1)) && !((uintptr_t)feats & 15);
    if (vec) hipLaunchKernelGGL((clip_score_kernel<T, 4>), g, dim3(256), 0, s, (const T*)img, (const T*)txt, feats, cosine, B, F, eps);
    else hipLaunchKernelGGL((clip_score_kernel<T, 1>), g, dim3(256), 0, s, (const T*)img, (const T*)txt, feats, cosine, B, F, eps);
    return sidlsg_last_error();
}

extern "C" {

int sidlsg_clip_patches_u8(const void* images, void* out, int B, int H, int W, int R, int P, int Kp, float mean0, float mean1, float mean2,
                           float std0, float std1, float std2, void* stream) {
    return clip_patches_t<bf16>(images, out, B, H, W, R, P, Kp, mean0, mean1, mean2, std0, std1, std2, stream);
}
int sidlsg_clip_patches_u8_f32(const void* images, void* out, int B, int H, int W, int R, int P, int Kp, float mean0, float mean1,
                               float mean2, float std0, float std1, float std2, void* stream) {
    return clip_patches_t<float>(images, out, B, H, W, R, P, Kp, mean0, mean1, mean2, std0, std1, std2, stream);
}

int sidlsg_gelu(const void* x, void* y, long long n, int mode, void* stream) { return clip_gelu_t<bf16>(x, y, n, mode, stream); }
int sidlsg_gelu_f32(const void* x, void* y, long long n, int mode, void* stream) { return clip_gelu_t<float>(x, y, n, mode, stream); }

int sidlsg_clip_score(const void* img, const void* txt, int f32_in, float* feats, float* cosine, int B, int F, void* stream) {
    if (!img || !txt || !feats || !cosine || B <= 0 || F <= 0 || (long long)B * 2 * F >= (1LL << 31)) return SIDLSG_EINVAL;
    return f32_in ? clip_score_t<float>(img, txt, feats, cosine, B, F, stream) : clip_score_t<bf16>(img, txt, feats, cosine, B, F, stream);
}

}  // extern "C"
