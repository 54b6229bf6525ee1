// The FID Inception-v3 detector on gfx950 (sid_lsg_amd/inception.py): its three kinds of launch, all fp32.  FID is a small
// difference of large statistics (the reason mmd.hip refuses 16-bit operands), and at the matrix fp32 rate the detector is far
// below the generation time of the images it scores, so there is no 16-bit variant.
//
//   sidlsg_conv2d_relu_f32     one general implicit-GEMM convolution (1x1, 3x3, 5x5, 1x7, 7x1, 1x3, 3x1; stride 1 | 2; any padding
//                              below the kernel size) with the folded BatchNorm shift as bias and an optional ReLU, on
//                              v_mfma_f32_16x16x4_f32: every output is an exact fp32 fma chain over k = (dh * KW + dw) * Cin + c
//                              in increasing k, then one add of the bias.  The output row stride is independent of Cout: a branch
//                              of an Inception block writes its channel slice of the block's output, no concat is formed.
//   sidlsg_pool2d_f32          max (padding never wins: the bits of F.max_pool2d) or mean over the taps inside the image
//                              (count_include_pad=False: row-major sum, one division), again with an output row stride.
//   sidlsg_inception_input_u8  uint8 NCHW -> [B][299][299][4] fp32: TF's legacy bilinear resize (source coordinate i * W / 299, no
//                              half-pixel offset, taps floor and +1 clamped to the border -- what the affine_grid / grid_sample pair
//                              of the published TorchScript detector computes), then (v - 128) / 128; channel 3 is zero.
//
// The convolution keeps the loop of fp32.hip's gemm_f32_kernel (64 x 64 tile, 16 k per LDS stage, register-staged loads, 2 x 2
// MFMA tiles per wave; A = weights so a lane ends with 4 consecutive output channels of one pixel).  What is new is the gather: a
// loader thread walks (dh, dw, c) of its 4-channel chunk forward by 16 k per stage instead of dividing, and padding is a bounds
// test that zero-fills.  This file is built with -ffp-contract=off: the lerps and the (v - 128) / 128 of the input kernel and the
// bias add of the epilogue are the roundings written here, not the compiler's fusion.
#include "common.h"

#define MFMA_F32(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

namespace {

constexpr int IC_BM = 64, IC_BN = 64, IC_BK = 16, IC_LD = IC_BK + 2;
constexpr int IC_SIDE = 299;
constexpr long long IC_LIM = 1LL << 31;

struct ConvParams {
    const float* X;      // [B][H][Wd][ldx]
    const float* W;      // [N][KH][KW][Cin] = [N][K]
    float* Y;            // [M][ldc], M = B * Ho * Wo
    const float* bias;   // [N]
    int ldx, ldc, M, N, K, H, Wd, Cin, Ho, Wo, KH, KW, stride, pad_h, pad_w, relu;
};

__global__ __launch_bounds__(256) void conv2d_relu_f32_kernel(ConvParams p) {
    __shared__ float Xs[IC_BM * IC_LD];
    __shared__ float Ws[IC_BN * IC_LD];
    const int tiles_n = (p.N + IC_BN - 1) / IC_BN;
    const int m0 = (blockIdx.x / tiles_n) * IC_BM, n0 = (blockIdx.x % tiles_n) * IC_BN;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lg = lane >> 4;
    const int wm0 = (wave >> 1) * 32, wn0 = (wave & 1) * 32;
    const int lrow = tid >> 2, lch = (tid & 3) * 4;          // loader: row of the tile, first of 4 consecutive k
    // the pixel this thread gathers for
    const int m = m0 + lrow;
    const bool mok = m < p.M;
    const int mm_ld = mok ? m : 0, hw = p.Ho * p.Wo;
    const int b = mm_ld / hw, rem = mm_ld - b * hw, ho = rem / p.Wo, wo = rem - ho * p.Wo;
    const size_t xbase = (size_t)b * p.H * p.Wd * p.ldx;
    const int hi0 = ho * p.stride - p.pad_h, wi0 = wo * p.stride - p.pad_w;
    // (dh, dw, c) of k = k0 + lch, advanced by IC_BK per stage; dh == KH: k is past K
    int c = lch, dh = 0, dw = 0;
    auto carry = [&]() {
        while (c >= p.Cin && dh < p.KH) {
            c -= p.Cin;
            if (++dw == p.KW) { dw = 0; dh++; }
        }
    };
    carry();
    const int n_ld = n0 + lrow;
    const bool nok = n_ld < p.N;
    const float* wrow = p.W + (size_t)(nok ? n_ld : 0) * p.K;
    auto load_x = [&]() -> f32x4 {
        f32x4 v = {0, 0, 0, 0};
        if (mok && dh < p.KH) {
            const int hi = hi0 + dh, wi = wi0 + dw;
            if (hi >= 0 && hi < p.H && wi >= 0 && wi < p.Wd) v = *reinterpret_cast<const f32x4*>(p.X + xbase + ((size_t)hi * p.Wd + wi) * p.ldx + c);
        }
        c += IC_BK;
        carry();
        return v;
    };
    auto load_w = [&](int k0) -> f32x4 {
        const int k = k0 + lch;
        if (!nok || k >= p.K) return (f32x4){0, 0, 0, 0};
        return *reinterpret_cast<const f32x4*>(wrow + k);
    };
    f32x4 acc[2][2];   // [n tile][m tile]
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) acc[i][j] = (f32x4){0, 0, 0, 0};
    const int nk = (p.K + IC_BK - 1) / IC_BK;
    f32x4 xr = load_x(), wr = load_w(0);
    for (int kt = 0; kt < nk; kt++) {
        __syncthreads();                                   // previous stage fully consumed
#pragma unroll
        for (int e = 0; e < 4; e++) { Xs[lrow * IC_LD + lch + e] = xr[e]; Ws[lrow * IC_LD + lch + e] = wr[e]; }
        __syncthreads();
        if (kt + 1 < nk) { xr = load_x(); wr = load_w((kt + 1) * IC_BK); }
#pragma unroll
        for (int k4 = 0; k4 < IC_BK / 4; k4++) {
            float fw[2], fx[2];
#pragma unroll
            for (int i = 0; i < 2; i++) fw[i] = Ws[(wn0 + i * 16 + li) * IC_LD + k4 * 4 + lg];
#pragma unroll
            for (int j = 0; j < 2; j++) fx[j] = Xs[(wm0 + j * 16 + li) * IC_LD + k4 * 4 + lg];
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int j = 0; j < 2; j++) acc[i][j] = MFMA_F32(fw[i], fx[j], acc[i][j]);
        }
    }
    // epilogue: the lane holds, for pixel mm = .. + li, channels n .. n + 3
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const int mm = m0 + wm0 + j * 16 + li;
        if (mm >= p.M) continue;
        float* yrow = p.Y + (size_t)mm * p.ldc;
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const int n = n0 + wn0 + i * 16 + lg * 4;
            if (n + 4 <= p.N) {
                const f32x4 bv = *reinterpret_cast<const f32x4*>(p.bias + n);
                f32x4 v = acc[i][j] + bv;
                if (p.relu) {
#pragma unroll
                    for (int r = 0; r < 4; r++) v[r] = v[r] > 0.f ? v[r] : 0.f;
                }
                *reinterpret_cast<f32x4*>(yrow + n) = v;
            } else {
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    if (n + r >= p.N) break;
                    float v = acc[i][j][r] + p.bias[n + r];
                    if (p.relu) v = v > 0.f ? v : 0.f;
                    yrow[n + r] = v;
                }
            }
        }
    }
}

struct PoolParams {
    const float* X;   // [B][H][W][ldx]
    float* Y;         // [B][Ho][Wo][ldy]
    int ldx, ldy, H, W, C4, Ho, Wo, k, stride, pad, mode;
    long long total;  // B * Ho * Wo * C4
};

// one thread per 4 channels of one output pixel
__global__ __launch_bounds__(256) void pool2d_f32_kernel(PoolParams p) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= p.total) return;
    const int c = (int)(t % p.C4) * 4;
    long long q = t / p.C4;
    const int wo = (int)(q % p.Wo);
    q /= p.Wo;
    const int ho = (int)(q % p.Ho), b = (int)(q / p.Ho);
    const int h0 = ho * p.stride - p.pad, w0 = wo * p.stride - p.pad;
    const float* xb = p.X + (size_t)b * p.H * p.W * p.ldx + c;
    f32x4 a = p.mode == 0 ? (f32x4){-INFINITY, -INFINITY, -INFINITY, -INFINITY} : (f32x4){0, 0, 0, 0};
    int count = 0;
    for (int dh = 0; dh < p.k; dh++) {
        const int hi = h0 + dh;
        if (hi < 0 || hi >= p.H) continue;
        for (int dw = 0; dw < p.k; dw++) {
            const int wi = w0 + dw;
            if (wi < 0 || wi >= p.W) continue;
            const f32x4 v = *reinterpret_cast<const f32x4*>(xb + ((size_t)hi * p.W + wi) * p.ldx);
            if (p.mode == 0) {
#pragma unroll
                for (int r = 0; r < 4; r++) a[r] = v[r] > a[r] ? v[r] : a[r];
            } else {
                a += v;
            }
            count++;
        }
    }
    if (p.mode == 1) {
        const float n = (float)count;
#pragma unroll
        for (int r = 0; r < 4; r++) a[r] = a[r] / n;
    }
    *reinterpret_cast<f32x4*>(p.Y + (((size_t)b * p.Ho + ho) * p.Wo + wo) * p.ldy + c) = a;
}

// one thread per output pixel: the source coordinate i * W / 299 exactly as quotient and remainder
__global__ __launch_bounds__(256) void inception_input_u8_kernel(const unsigned char* __restrict__ img, float* __restrict__ out, int B, int H, int W) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)B * IC_SIDE * IC_SIDE) return;
    const int ox = (int)(t % IC_SIDE);
    const long long q = t / IC_SIDE;
    const int oy = (int)(q % IC_SIDE), b = (int)(q / IC_SIDE);
    const int px = ox * W, py = oy * H;
    const int x0 = px / IC_SIDE, y0 = py / IC_SIDE;
    const float lx = (float)(px - x0 * IC_SIDE) / 299.0f, ly = (float)(py - y0 * IC_SIDE) / 299.0f;
    const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
    f32x4 v = {0, 0, 0, 0};
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        const unsigned char* pl = img + ((size_t)b * 3 + ch) * H * W;
        const float a00 = (float)pl[(size_t)y0 * W + x0], a01 = (float)pl[(size_t)y0 * W + x1];
        const float a10 = (float)pl[(size_t)y1 * W + x0], a11 = (float)pl[(size_t)y1 * W + x1];
        const float top = a00 + lx * (a01 - a00), bot = a10 + lx * (a11 - a10);     // horizontal, then vertical
        const float r = top + ly * (bot - top);
        v[ch] = (r - 128.0f) / 128.0f;
    }
    *reinterpret_cast<f32x4*>(out + (size_t)t * 4) = v;
}

bool ic_kernel_side(int k) { return k == 1 || k == 3 || k == 5 || k == 7; }

}  // namespace

extern "C" {

int sidlsg_conv2d_relu_f32(const float* X, int ldx, const float* W, float* Y, int ldc, const float* bias, int B, int H, int Wd, int Cin,
                           int Cout, int KH, int KW, int stride, int pad_h, int pad_w, int relu, void* stream) {
    if (!X || !W || !Y || !bias || (((uintptr_t)X | (uintptr_t)W | (uintptr_t)Y | (uintptr_t)bias) & 15)) return SIDLSG_EINVAL;
    if (B < 1 || H < 1 || Wd < 1 || Cin < 4 || (Cin & 3) || Cout < 1 || (ldx & 3) || (ldc & 3) || ldx < Cin || ldc < Cout) return SIDLSG_EINVAL;
    if (!ic_kernel_side(KH) || !ic_kernel_side(KW) || !(KH == KW ? KH <= 5 : (KH == 1 || KW == 1) && KH + KW != 6)) return SIDLSG_EINVAL;
    if ((stride != 1 && stride != 2) || pad_h < 0 || pad_h >= KH || pad_w < 0 || pad_w >= KW) return SIDLSG_EINVAL;
    if (H + 2 * pad_h < KH || Wd + 2 * pad_w < KW) return SIDLSG_EINVAL;
    ConvParams p;
    p.Ho = (H + 2 * pad_h - KH) / stride + 1;
    p.Wo = (Wd + 2 * pad_w - KW) / stride + 1;
    const long long M = (long long)B * p.Ho * p.Wo, K = (long long)KH * KW * Cin;
    if ((long long)B * H * Wd * ldx * 4 >= IC_LIM || M * ldc * 4 >= IC_LIM || K * Cout * 4 >= IC_LIM) return SIDLSG_EINVAL;
    const long long tiles = ((M + IC_BM - 1) / IC_BM) * ((Cout + IC_BN - 1) / IC_BN);
    if (tiles >= IC_LIM) return SIDLSG_EINVAL;
    p.X = X; p.W = W; p.Y = Y; p.bias = bias; p.ldx = ldx; p.ldc = ldc; p.M = (int)M; p.N = Cout; p.K = (int)K; p.H = H; p.Wd = Wd;
    p.Cin = Cin; p.KH = KH; p.KW = KW; p.stride = stride; p.pad_h = pad_h; p.pad_w = pad_w; p.relu = relu ? 1 : 0;
    hipLaunchKernelGGL(conv2d_relu_f32_kernel, dim3((unsigned)tiles), dim3(256), 0, (hipStream_t)stream, p);
    return sidlsg_last_error();
}

int sidlsg_pool2d_f32(const float* X, int ldx, float* Y, int ldy, int B, int H, int W, int C, int k, int stride, int pad, int mode,
                      void* stream) {
    if (!X || !Y || (((uintptr_t)X | (uintptr_t)Y) & 15)) return SIDLSG_EINVAL;
    if (B < 1 || H < 1 || W < 1 || C < 4 || (C & 3) || (ldx & 3) || (ldy & 3) || ldx < C || ldy < C) return SIDLSG_EINVAL;
    if (k < 1 || k > 8 || stride < 1 || pad < 0 || 2 * pad > k || H + 2 * pad < k || W + 2 * pad < k || mode < 0 || mode > 1) return SIDLSG_EINVAL;
    PoolParams p;
    p.Ho = (H + 2 * pad - k) / stride + 1;
    p.Wo = (W + 2 * pad - k) / stride + 1;
    if ((long long)B * H * W * ldx * 4 >= IC_LIM || (long long)B * p.Ho * p.Wo * ldy * 4 >= IC_LIM) return SIDLSG_EINVAL;
    p.X = X; p.Y = Y; p.ldx = ldx; p.ldy = ldy; p.H = H; p.W = W; p.C4 = C / 4; p.k = k; p.stride = stride; p.pad = pad; p.mode = mode;
    p.total = (long long)B * p.Ho * p.Wo * p.C4;
    hipLaunchKernelGGL(pool2d_f32_kernel, dim3((unsigned)((p.total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p);
    return sidlsg_last_error();
}

int sidlsg_inception_input_u8(const void* images, float* out, int B, int H, int W, void* stream) {
    if (!images || !out || ((uintptr_t)out & 15) || B < 1 || H < 1 || W < 1 || H > 16384 || W > 16384) return SIDLSG_EINVAL;
    const long long pixels = (long long)B * IC_SIDE * IC_SIDE;
    if ((long long)B * 3 * H * W >= IC_LIM || pixels * 16 >= IC_LIM) return SIDLSG_EINVAL;
    hipLaunchKernelGGL(inception_input_u8_kernel, dim3((unsigned)((pixels + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned char*)images, out, B, H, W);
    return sidlsg_last_error();
}

}  // extern "C"
