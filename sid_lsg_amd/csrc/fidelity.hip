// Paired image fidelity on gfx950: PSNR / SSIM of two uint8 image sets in one pass, and the two kernels LPIPS adds to the fp32
// convolution path (the input conversion and the per-tap distance).  Forward only.
// Compiled with -ffp-contract=off (csrc/build.py EXTRA): every operation below is rounded once, in the order written.
//
// No atomics and no data-dependent loops: each workgroup writes its partial sums to its own workspace slots, and a second launch adds
// the slots of an image in a fixed order (mmd.hip's scheme).  The same inputs give the same bits on every run.
#include "common.h"
#include <cmath>

namespace {

// ---- PSNR / SSIM ----------------------------------------------------------------------------------------------------------------
// One workgroup = one (image, channel, tile of FD_TH x FD_TW pixel POSITIONS of the full H x W image).  A position is a term of the
// squared error, and it is the centre of an SSIM window when 5 <= y < H - 5 and 5 <= x < W - 5; the mask is read at the position, so a
// kept SSIM term is a window whose centre pixel is kept.  The uint8 tile and its halo of 5 go to LDS (positions outside the image are
// staged as 0 and only ever reach windows that are not counted), the horizontal pass leaves the five row moments in LDS as doubles,
// the vertical pass and the SSIM formula run per position in fp64.
constexpr int FD_R = 5, FD_K = 2 * FD_R + 1;
constexpr int FD_TW = 32, FD_TH = 16;
constexpr int FD_IW = FD_TW + 2 * FD_R, FD_IH = FD_TH + 2 * FD_R;      // 42 x 26 staged pixels
constexpr int FD_Q = 8;                                                // quantities per image
constexpr double FD_C1 = (0.01 * 255.0) * (0.01 * 255.0), FD_C2 = (0.03 * 255.0) * (0.03 * 255.0);

struct FdWin { double g[FD_K]; };

struct FdSmem {
    unsigned char px[2][FD_IH][FD_IW + 2];      // a, b
    double hz[5][FD_IH][FD_TW];                 // x, y, xx, yy, xy after the horizontal pass: 33280 bytes
    double red[4][FD_Q];
};

DEVFN double fd_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// grid = (tiles of one plane, B * 3).  ws[((image * 3 + channel) * ntiles + tile) * 8 + q]
__global__ __launch_bounds__(256) void fd_psnr_ssim_kernel(const uint8_t* __restrict__ A, const uint8_t* __restrict__ Bm, const uint8_t* __restrict__ mask,
                                                           int H, int W, int tiles_x, int ntiles, FdWin win, double* __restrict__ ws) {
    __shared__ FdSmem sm;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int plane = blockIdx.y, img = plane / 3, tile = blockIdx.x;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int y0 = ty * FD_TH, x0 = tx * FD_TW;
    const size_t pbase = (size_t)plane * H * W;
    for (int i = t; i < FD_IH * FD_IW; i += 256) {
        const int r = i / FD_IW, c = i - r * FD_IW;
        const int y = y0 - FD_R + r, x = x0 - FD_R + c;
        unsigned char va = 0, vb = 0;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            va = A[pbase + (size_t)y * W + x];
            vb = Bm[pbase + (size_t)y * W + x];
        }
        sm.px[0][r][c] = va;
        sm.px[1][r][c] = vb;
    }
    __syncthreads();
    for (int i = t; i < FD_IH * FD_TW; i += 256) {
        const int r = i / FD_TW, c = i - r * FD_TW;
        double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
#pragma unroll
        for (int k = 0; k < FD_K; k++) {
            const double g = win.g[k];
            const double x = (double)sm.px[0][r][c + k], y = (double)sm.px[1][r][c + k];
            sx += g * x;
            sy += g * y;
            sxx += g * (x * x);
            syy += g * (y * y);
            sxy += g * (x * y);
        }
        sm.hz[0][r][c] = sx;
        sm.hz[1][r][c] = sy;
        sm.hz[2][r][c] = sxx;
        sm.hz[3][r][c] = syy;
        sm.hz[4][r][c] = sxy;
    }
    __syncthreads();
    double q[FD_Q];
#pragma unroll
    for (int k = 0; k < FD_Q; k++) q[k] = 0.0;
#pragma unroll
    for (int rep = 0; rep < FD_TH * FD_TW / 256; rep++) {
        const int i = t + 256 * rep;
        const int r = i / FD_TW, c = i - r * FD_TW;
        const int y = y0 + r, x = x0 + c;
        const bool in = y < H && x < W;
        const bool centre = in && y >= FD_R && y < H - FD_R && x >= FD_R && x < W - FD_R;
        bool kept = in;
        if (in && mask) kept = mask[((size_t)img * H + y) * W + x] < 128;
        const double d = (double)((int)sm.px[0][r + FD_R][c + FD_R] - (int)sm.px[1][r + FD_R][c + FD_R]);
        const double se = in ? d * d : 0.0;
        double mx = 0.0, my = 0.0, exx = 0.0, eyy = 0.0, exy = 0.0;
#pragma unroll
        for (int k = 0; k < FD_K; k++) {
            const double g = win.g[k];
            mx += g * sm.hz[0][r + k][c];
            my += g * sm.hz[1][r + k][c];
            exx += g * sm.hz[2][r + k][c];
            eyy += g * sm.hz[3][r + k][c];
            exy += g * sm.hz[4][r + k][c];
        }
        const double mxx = mx * mx, myy = my * my, mxy = mx * my;
        const double vx = exx - mxx, vy = eyy - myy, cxy = exy - mxy;
        const double num = (2.0 * mxy + FD_C1) * (2.0 * cxy + FD_C2);
        const double den = ((mxx + myy) + FD_C1) * ((vx + vy) + FD_C2);
        const double s = centre ? num / den : 0.0;
        q[0] += se;
        q[1] += in ? 1.0 : 0.0;
        q[2] += s;
        q[3] += centre ? 1.0 : 0.0;
        q[4] += kept ? se : 0.0;
        q[5] += kept ? 1.0 : 0.0;
        q[6] += kept ? s : 0.0;
        q[7] += (kept && centre) ? 1.0 : 0.0;
    }
#pragma unroll
    for (int k = 0; k < FD_Q; k++) {
        const double v = fd_wave_sum(q[k]);
        if (lane == 0) sm.red[wave][k] = v;
    }
    __syncthreads();
    if (t < FD_Q) ws[((size_t)plane * ntiles + tile) * FD_Q + t] = ((sm.red[0][t] + sm.red[1][t]) + sm.red[2][t]) + sm.red[3][t];
}

// out[image][q] = the image's `slots` workspace entries of quantity q: thread t adds entries t, t + 256, .. in that order, then the
// 256 partial sums are added pairwise in a fixed tree.  grid = (8, B).
__global__ __launch_bounds__(256) void fd_reduce_kernel(const double* __restrict__ ws, double* __restrict__ out, int slots) {
    __shared__ double part[256];
    const int q = blockIdx.x, img = blockIdx.y, t = threadIdx.x;
    const double* w = ws + (size_t)img * slots * FD_Q + q;
    double s = 0.0;
    for (int i = t; i < slots; i += 256) s += w[(size_t)i * FD_Q];
    part[t] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) part[t] += part[t + o];
        __syncthreads();
    }
    if (t == 0) out[img * FD_Q + q] = part[0];
}

// tiles of one plane; false for sizes the entry point rejects
bool fd_geometry(int B, int H, int W, int* tiles_x, int* ntiles) {
    if (B < 1 || B > 21845 || H < FD_K || W < FD_K) return false;
    if ((long long)B * 3 * H * W >= (1LL << 31)) return false;
    const long long tx = (W + FD_TW - 1) / FD_TW, ty = (H + FD_TH - 1) / FD_TH;
    if (tx * ty * 3 * B * FD_Q >= (1LL << 31)) return false;
    *tiles_x = (int)tx;
    *ntiles = (int)(tx * ty);
    return true;
}

// ---- LPIPS input ----------------------------------------------------------------------------------------------------------------
struct LpNorm { float shift[3], scale[3]; };

// one thread = one pixel of one image of the batch of 2B
__global__ __launch_bounds__(256) void lp_input_kernel(const uint8_t* __restrict__ A, const uint8_t* __restrict__ Bm, float* __restrict__ out, int B,
                                                       int HW, LpNorm nrm) {
    const int p = blockIdx.x * 256 + threadIdx.x, row = blockIdx.y;
    if (p >= HW) return;
    const uint8_t* src = (row < B ? A + (size_t)row * 3 * HW : Bm + (size_t)(row - B) * 3 * HW) + p;
    f32x4 v;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        float tt = __fdiv_rn((float)src[(size_t)c * HW], 127.5f);
        tt = __fsub_rn(tt, 1.0f);
        v[c] = __fdiv_rn(__fsub_rn(tt, nrm.shift[c]), nrm.scale[c]);
    }
    v[3] = 0.0f;
    *reinterpret_cast<f32x4*>(out + ((size_t)row * HW + p) * 4) = v;
}

// ---- LPIPS layer ----------------------------------------------------------------------------------------------------------------
// 16 lanes = one pixel: lane l of the group owns the 16-byte chunks l, l + 16, .. of the pixel's C channels.  Every C-term sum (the
// two sums of squares and the weighted sum) is: per lane its elements in increasing channel order, one fp32 accumulator; then the
// 16 lanes by an xor butterfly (8, 4, 2, 1), which leaves the same bits in every lane.  A group walks LP_PPG pixels and adds their
// values in double; the 16 groups of a workgroup are added in order; one slot per workgroup.
constexpr int LP_PPG = 8, LP_PPB = 16 * LP_PPG;

DEVFN float lp_group_sum(float v) {
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v = __fadd_rn(v, __shfl_xor(v, o, 64));
    return v;
}

// the 128-pixel block blockIdx.x of the maps F0 and F1 -> *slot; 256 threads
DEVFN void lp_pair_block(const float* __restrict__ F0, const float* __restrict__ F1, int ldf, const float* __restrict__ w, int npix, int C,
                         double* __restrict__ slot) {
    __shared__ double red[16];
    const int t = threadIdx.x, l = t & 15, grp = t >> 4, c4 = C >> 2;
    double acc = 0.0;
    for (int j = 0; j < LP_PPG; j++) {
        const int p = blockIdx.x * LP_PPB + j * 16 + grp;
        float val;
        {                                                     // a group past the last pixel recomputes it and drops the value: no divergent shuffle
            const float* f0 = F0 + (size_t)min(p, npix - 1) * ldf;
            const float* f1 = F1 + (size_t)min(p, npix - 1) * ldf;
            float s0 = 0.0f, s1 = 0.0f;
            for (int k = l; k < c4; k += 16) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(f0 + 4 * k), b = *reinterpret_cast<const f32x4*>(f1 + 4 * k);
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    s0 = __fadd_rn(s0, __fmul_rn(a[e], a[e]));
                    s1 = __fadd_rn(s1, __fmul_rn(b[e], b[e]));
                }
            }
            s0 = lp_group_sum(s0);
            s1 = lp_group_sum(s1);
            const float n0 = __fadd_rn(__fsqrt_rn(s0), 1e-10f), n1 = __fadd_rn(__fsqrt_rn(s1), 1e-10f);
            float sd = 0.0f;
            for (int k = l; k < c4; k += 16) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(f0 + 4 * k), b = *reinterpret_cast<const f32x4*>(f1 + 4 * k);
                const f32x4 wk = *reinterpret_cast<const f32x4*>(w + 4 * k);
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const float d = __fsub_rn(__fdiv_rn(a[e], n0), __fdiv_rn(b[e], n1));
                    sd = __fadd_rn(sd, __fmul_rn(wk[e], __fmul_rn(d, d)));
                }
            }
            val = lp_group_sum(sd);
        }
        acc += p < npix ? (double)val : 0.0;
    }
    if (l == 0) red[grp] = acc;
    __syncthreads();
    if (t == 0) {
        double s = 0.0;
#pragma unroll
        for (int g = 0; g < 16; g++) s += red[g];
        *slot = s;
    }
}

// grid = (pixel blocks, B).  ws[image * nblk + block]
__global__ __launch_bounds__(256) void lp_layer_kernel(const float* __restrict__ F, int ldf, const float* __restrict__ w, int B, int npix, int C,
                                                       int nblk, double* __restrict__ ws) {
    const int img = blockIdx.y;
    lp_pair_block(F + (size_t)img * npix * ldf, F + (size_t)(B + img) * npix * ldf, ldf, w, npix, C, ws + (size_t)img * nblk + blockIdx.x);
}

// out[image] = (the image's nblk slots, added as in fd_reduce_kernel) / npix.  grid = B.
__global__ __launch_bounds__(256) void lp_reduce_kernel(const double* __restrict__ ws, double* __restrict__ out, int nblk, int npix) {
    __shared__ double part[256];
    const int img = blockIdx.x, t = threadIdx.x;
    const double* w = ws + (size_t)img * nblk;
    double s = 0.0;
    for (int i = t; i < nblk; i += 256) s += w[i];
    part[t] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) part[t] += part[t + o];
        __syncthreads();
    }
    if (t == 0) out[img] = part[0] / (double)npix;
}

// out[i] = ((v[0][i] + v[1][i]) + v[2][i]) + ..: the taps of a pair in order, whatever batch the pair travels in
__global__ __launch_bounds__(256) void lp_sum_kernel(const double* __restrict__ v, int taps, int B, double* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B) return;
    double s = v[i];
    for (int k = 1; k < taps; k++) s += v[(size_t)k * B + i];
    out[i] = s;
}

// ---- LPIPS group: all pairs of K images ---------------------------------------------------------------------------------------------
// Two launch forms that write the same bits, those of lp_layer_kernel for each pair.
//
// lp_group_pair_kernel spreads the pairs over the grid: block (x, pair, g) is lp_layer_kernel's block x for the rows gK + i and gK + j
// of the pair, without the gathered copies.  Every map is read K - 1 times, from L2 at the sizes this form is taken for.
//
// lp_group_kernel forms all pairs of a 128-pixel block in one workgroup, so F is read once: f / n does not depend on the partner, so
// every vector is normalised once; d * d is symmetric, so only i < j is formed.  A lane only ever touches its own 16-byte chunks
// (l, l + 16, ..) of the K vectors of a pixel, so the normalised copy in LDS is lane-private: qs[(image * nch + chunk) * T + thread],
// one ds_read_b128 per chunk, no bank conflict and no barrier.  Per pair and lane group one double in LDS (accs[pair][group]), added
// to by lane 0 of the group alone in pixel order; thread `pair` adds the 16 groups in order into the pair's slot of this block.  The
// block has T = 256 or 128 threads (the larger whose copy fits next to the accumulators) and walks the 16 lane groups of the pixel
// block in 256 / T rounds.  NCH > 0: a lane owns at most NCH chunks (C <= 64 NCH) and the chunk loops are unrolled, image i's chunks
// and the weights held in registers; NCH == 0: any C, loops over nch chunks.
constexpr int LPG_KMAX = 16, LPG_LDS = 64 * 1024, LPG_MIN_BLOCKS = 512;

// grid = (pixel blocks, P, G).  ws[(g * P + pair) * nblk + block]
__global__ __launch_bounds__(256) void lp_group_pair_kernel(const float* __restrict__ F, int ldf, const float* __restrict__ w, int K, int npix, int C,
                                                            int nblk, double* __restrict__ ws) {
    int i = 0, first = 0;                                     // pair -> (i, j): row i holds the pairs first .. first + K - 2 - i
    while ((int)blockIdx.y >= first + K - 1 - i) {
        first += K - 1 - i;
        i++;
    }
    const int j = i + 1 + ((int)blockIdx.y - first);
    const float* Fg = F + (size_t)blockIdx.z * K * npix * ldf;
    lp_pair_block(Fg + (size_t)i * npix * ldf, Fg + (size_t)j * npix * ldf, ldf, w, npix, C,
                  ws + ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * nblk + blockIdx.x);
}

// grid = (pixel blocks, G), T threads, P * 128 + K * nch * T * 16 bytes of LDS.  ws[(g * P + pair) * nblk + block]
template <int NCH>
__global__ __launch_bounds__(256) void lp_group_kernel(const float* __restrict__ F, int ldf, const float* __restrict__ w, int K, int npix, int C,
                                                       int nblk, int nch, double* __restrict__ ws) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lpg_smem[];
    const int T = blockDim.x, t = threadIdx.x, l = t & 15, c4 = C >> 2, P = K * (K - 1) / 2;
    const int nc = NCH > 0 ? NCH : nch;
    constexpr int LPG_UNROLL = NCH > 0 ? NCH : 1;                                        // the chunk loops: whole when NCH is known
    double* accs = reinterpret_cast<double*>(lpg_smem);                                  // [P][16]
    f32x4* qs = reinterpret_cast<f32x4*>(lpg_smem + (size_t)P * 16 * sizeof(double));    // [K][nch][T]
    for (int i = t; i < P * 16; i += T) accs[i] = 0.0;
    __syncthreads();
    const size_t istride = (size_t)npix * ldf;
    const float* Fg = F + (size_t)blockIdx.y * K * istride;
    f32x4 wreg[NCH > 0 ? NCH : 1], areg[NCH > 0 ? NCH : 1];
    if (NCH > 0) {
#pragma unroll LPG_UNROLL
        for (int c = 0; c < nc; c++) {
            const int k = l + 16 * c;
            if (k < c4) wreg[c] = *reinterpret_cast<const f32x4*>(w + 4 * k);
        }
    }
    for (int g0 = 0; g0 < 16; g0 += T >> 4) {
        const int grp = g0 + (t >> 4);
        for (int j = 0; j < LP_PPG; j++) {
            const int p = blockIdx.x * LP_PPB + j * 16 + grp;
            const float* f = Fg + (size_t)min(p, npix - 1) * ldf;     // a group past the last pixel recomputes it and drops the values
            for (int i = 0; i < K; i++) {                             // the K vectors of the pixel, normalised, into this lane's slots
                const float* fi = f + (size_t)i * istride;
                float s = 0.0f;
#pragma unroll LPG_UNROLL
                for (int c = 0; c < nc; c++) {
                    const int k = l + 16 * c;
                    if (k < c4) {
                        const f32x4 a = *reinterpret_cast<const f32x4*>(fi + 4 * k);
                        qs[(size_t)(i * nch + c) * T + t] = a;
#pragma unroll
                        for (int e = 0; e < 4; e++) s = __fadd_rn(s, __fmul_rn(a[e], a[e]));
                    }
                }
                s = lp_group_sum(s);
                const float n = __fadd_rn(__fsqrt_rn(s), 1e-10f);
#pragma unroll LPG_UNROLL
                for (int c = 0; c < nc; c++) {
                    const int k = l + 16 * c;
                    if (k < c4) {
                        f32x4 a = qs[(size_t)(i * nch + c) * T + t];
#pragma unroll
                        for (int e = 0; e < 4; e++) a[e] = __fdiv_rn(a[e], n);
                        qs[(size_t)(i * nch + c) * T + t] = a;
                    }
                }
            }
            int pair = 0;
            for (int i = 0; i < K - 1; i++) {
                if (NCH > 0) {
#pragma unroll LPG_UNROLL
                    for (int c = 0; c < nc; c++) {
                        const int k = l + 16 * c;
                        if (k < c4) areg[c] = qs[(size_t)(i * nch + c) * T + t];
                    }
                }
                for (int jj = i + 1; jj < K; jj++, pair++) {
                    float sd = 0.0f;
#pragma unroll LPG_UNROLL
                    for (int c = 0; c < nc; c++) {
                        const int k = l + 16 * c;
                        if (k < c4) {
                            const f32x4 a = NCH > 0 ? areg[c] : qs[(size_t)(i * nch + c) * T + t];
                            const f32x4 wk = NCH > 0 ? wreg[c] : *reinterpret_cast<const f32x4*>(w + 4 * k);
                            const f32x4 b = qs[(size_t)(jj * nch + c) * T + t];
#pragma unroll
                            for (int e = 0; e < 4; e++) {
                                const float d = __fsub_rn(a[e], b[e]);
                                sd = __fadd_rn(sd, __fmul_rn(wk[e], __fmul_rn(d, d)));
                            }
                        }
                    }
                    const float val = lp_group_sum(sd);
                    if (l == 0) accs[pair * 16 + grp] += p < npix ? (double)val : 0.0;
                }
            }
        }
    }
    __syncthreads();
    for (int pr = t; pr < P; pr += T) {
        double s = 0.0;
#pragma unroll
        for (int g = 0; g < 16; g++) s += accs[pr * 16 + g];
        ws[((size_t)blockIdx.y * P + pr) * nblk + blockIdx.x] = s;
    }
}

// the admitted set of sidlsg_lpips_group_f32 but for the pointers: pixel blocks, or false
bool lpg_geometry(int G, int K, int h, int wd, int* nblk) {
    if (K < 2 || K > LPG_KMAX || G < 1 || h < 1 || wd < 1) return false;
    const long long P = (long long)K * (K - 1) / 2;
    if ((long long)G * K > 32767 || (long long)G * P > 32767) return false;
    const long long npix = (long long)h * wd;
    if (npix >= (1LL << 31)) return false;
    const long long nb = (npix + LP_PPB - 1) / LP_PPB;
    if (nb * G * P >= (1LL << 31)) return false;
    *nblk = (int)nb;
    return true;
}

// threads of lp_group_kernel: the larger of 256 and 128 whose normalised copy fits next to the accumulators, or 0 (the copy does
// not fit: C 128 from K 14, C 256 from K 8, C 512 from K 4)
int lpg_threads(int K, int nch) {
    const size_t accs = (size_t)(K * (K - 1) / 2) * 16 * sizeof(double);
    for (int T = 256; T >= 128; T >>= 1)
        if (accs + (size_t)K * nch * T * 16 <= (size_t)LPG_LDS) return T;
    return 0;
}

bool lp_geometry(int B, int h, int wd, int* nblk) {
    if (B < 1 || B > 32767 || h < 1 || wd < 1) return false;
    const long long npix = (long long)h * wd;
    if (npix >= (1LL << 31)) return false;
    const long long nb = (npix + LP_PPB - 1) / LP_PPB;
    if (nb * B >= (1LL << 31)) return false;
    *nblk = (int)nb;
    return true;
}

}  // namespace

extern "C" {

int sidlsg_psnr_ssim_ws_doubles(int B, int H, int W) {
    int tiles_x, ntiles;
    if (!fd_geometry(B, H, W, &tiles_x, &ntiles)) return -1;
    return B * 3 * ntiles * FD_Q;
}

int sidlsg_psnr_ssim_u8(const void* a, const void* b, const void* mask, int B, int H, int W, double* out, double* ws, void* stream) {
    int tiles_x, ntiles;
    if (!a || !b || !out || !ws || ((uintptr_t)out & 7) || ((uintptr_t)ws & 7)) return SIDLSG_EINVAL;
    if (!fd_geometry(B, H, W, &tiles_x, &ntiles)) return SIDLSG_EINVAL;
    FdWin win;
    double sum = 0.0;
    for (int k = 0; k < FD_K; k++) {
        const double x = (double)(k - FD_R);
        win.g[k] = std::exp(-(x * x) / (2.0 * 1.5 * 1.5));
        sum += win.g[k];
    }
    for (int k = 0; k < FD_K; k++) win.g[k] /= sum;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(fd_psnr_ssim_kernel, dim3((unsigned)ntiles, (unsigned)(B * 3)), dim3(256), 0, s, (const uint8_t*)a, (const uint8_t*)b,
                       (const uint8_t*)mask, H, W, tiles_x, ntiles, win, ws);
    hipLaunchKernelGGL(fd_reduce_kernel, dim3(FD_Q, (unsigned)B), dim3(256), 0, s, (const double*)ws, out, 3 * ntiles);
    return sidlsg_last_error();
}

int sidlsg_lpips_input_u8(const void* a, const void* b, float* out, int B, int H, int W, float shift0, float shift1, float shift2, float scale0,
                          float scale1, float scale2, void* stream) {
    if (!a || !b || !out || ((uintptr_t)out & 15) || B < 1 || B > 32767 || H < 1 || W < 1) return SIDLSG_EINVAL;
    if (!(scale0 != 0.0f) || !(scale1 != 0.0f) || !(scale2 != 0.0f)) return SIDLSG_EINVAL;
    const long long hw = (long long)H * W;
    if (2 * (long long)B * hw * 16 >= (1LL << 31)) return SIDLSG_EINVAL;
    const LpNorm nrm = {{shift0, shift1, shift2}, {scale0, scale1, scale2}};
    hipLaunchKernelGGL(lp_input_kernel, dim3((unsigned)((hw + 255) / 256), (unsigned)(2 * B)), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)a,
                       (const uint8_t*)b, out, B, (int)hw, nrm);
    return sidlsg_last_error();
}

int sidlsg_lpips_layer_ws_doubles(int B, int h, int wd) {
    int nblk;
    if (!lp_geometry(B, h, wd, &nblk)) return -1;
    return B * nblk;
}

int sidlsg_lpips_layer_f32(const float* F, int ldf, const float* w, int B, int h, int wd, int C, double* out, double* ws, void* stream) {
    int nblk;
    if (!F || !w || !out || !ws || (((uintptr_t)F | (uintptr_t)w) & 15) || (((uintptr_t)out | (uintptr_t)ws) & 7)) return SIDLSG_EINVAL;
    if (C < 4 || (C & 3) || ldf < C || (ldf & 3)) return SIDLSG_EINVAL;
    if (!lp_geometry(B, h, wd, &nblk)) return SIDLSG_EINVAL;
    const long long npix = (long long)h * wd;
    if (2 * (long long)B * npix * ldf * 4 >= (1LL << 31)) return SIDLSG_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(lp_layer_kernel, dim3((unsigned)nblk, (unsigned)B), dim3(256), 0, s, F, ldf, w, B, (int)npix, C, nblk, ws);
    hipLaunchKernelGGL(lp_reduce_kernel, dim3((unsigned)B), dim3(256), 0, s, (const double*)ws, out, nblk, (int)npix);
    return sidlsg_last_error();
}

int sidlsg_lpips_group_ws_doubles(int G, int K, int h, int wd) {
    int nblk;
    if (!lpg_geometry(G, K, h, wd, &nblk)) return -1;
    return G * (K * (K - 1) / 2) * nblk;
}

int sidlsg_lpips_group_form_f32(const float* F, int ldf, const float* w, int G, int K, int h, int wd, int C, int form, double* out, double* ws,
                                void* stream);

int sidlsg_lpips_group_f32(const float* F, int ldf, const float* w, int G, int K, int h, int wd, int C, double* out, double* ws, void* stream) {
    return sidlsg_lpips_group_form_f32(F, ldf, w, G, K, h, wd, C, 0, out, ws, stream);
}

int sidlsg_lpips_group_form_f32(const float* F, int ldf, const float* w, int G, int K, int h, int wd, int C, int form, double* out, double* ws,
                                void* stream) {
    int nblk;
    if (form < 0 || form > 2) return SIDLSG_EINVAL;
    if (!F || !w || !out || !ws || (((uintptr_t)F | (uintptr_t)w) & 15) || (((uintptr_t)out | (uintptr_t)ws) & 7)) return SIDLSG_EINVAL;
    if (C < 4 || (C & 3) || ldf < C || (ldf & 3)) return SIDLSG_EINVAL;
    if (!lpg_geometry(G, K, h, wd, &nblk)) return SIDLSG_EINVAL;
    const long long npix = (long long)h * wd;
    if ((long long)G * K * npix * ldf * 4 >= (1LL << 31)) return SIDLSG_EINVAL;
    const int P = K * (K - 1) / 2, nch = ((C >> 2) + 15) / 16, T = lpg_threads(K, nch);
    if (form == 1 && !T) return SIDLSG_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    // The on-chip form reads F once, but each of its workgroups walks the P pairs of its pixels in turn: with fewer than LPG_MIN_BLOCKS
    // workgroups most of the 256 CUs idle (128 workgroups at 128 x 128, K 4: 3.6 times the paired launch; profiles/diversity.txt).
    // Such maps, and groups whose normalised copy does not fit in LDS, spread the pairs over the grid.
    if (form == 2 || (form == 0 && (!T || (long long)nblk * G < LPG_MIN_BLOCKS))) {
        hipLaunchKernelGGL(lp_group_pair_kernel, dim3((unsigned)nblk, (unsigned)P, (unsigned)G), dim3(256), 0, s, F, ldf, w, K, (int)npix, C, nblk, ws);
    } else {
        const size_t lds = (size_t)P * 16 * sizeof(double) + (size_t)K * nch * T * 16;
        const dim3 grid((unsigned)nblk, (unsigned)G);
        if (nch <= 1) hipLaunchKernelGGL(lp_group_kernel<1>, grid, dim3(T), lds, s, F, ldf, w, K, (int)npix, C, nblk, nch, ws);
        else if (nch <= 2) hipLaunchKernelGGL(lp_group_kernel<2>, grid, dim3(T), lds, s, F, ldf, w, K, (int)npix, C, nblk, nch, ws);
        else if (nch <= 4) hipLaunchKernelGGL(lp_group_kernel<4>, grid, dim3(T), lds, s, F, ldf, w, K, (int)npix, C, nblk, nch, ws);
        else if (nch <= 8) hipLaunchKernelGGL(lp_group_kernel<8>, grid, dim3(T), lds, s, F, ldf, w, K, (int)npix, C, nblk, nch, ws);
        else hipLaunchKernelGGL(lp_group_kernel<0>, grid, dim3(T), lds, s, F, ldf, w, K, (int)npix, C, nblk, nch, ws);
    }
    hipLaunchKernelGGL(lp_reduce_kernel, dim3((unsigned)(G * P)), dim3(256), 0, s, (const double*)ws, out, nblk, (int)npix);
    return sidlsg_last_error();
}

int sidlsg_lpips_sum_f64(const double* vals, int taps, int B, double* out, void* stream) {
    if (!vals || !out || (((uintptr_t)vals | (uintptr_t)out) & 7) || taps < 1 || taps > 64 || B < 1 || B > 32767) return SIDLSG_EINVAL;
    hipLaunchKernelGGL(lp_sum_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, (hipStream_t)stream, vals, taps, B, out);
    return sidlsg_last_error();
}

}  // extern "C"
