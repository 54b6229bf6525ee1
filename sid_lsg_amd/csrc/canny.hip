// Canny edge maps and edge-set matching for the ControlNet paths (gfx950): the Canny annotator's control image made on the device, and
// the counts behind the edge-adherence figure (sid_lsg_amd/edges.py).  Integer arithmetic throughout; include/sidlsg_hip.h holds the rules.
// Edge sets are bit planes, uint32 [B][H][Wd], Wd = ceil(W / 32), pixel x = bit x % 32 of word x / 32, padding bits 0: a wave64 ballot is
// two words of a plane, a 3 x 3 dilation is shifts and ORs, a count is a popcount, and both planes of a 768 x 768 image fit in one CU's LDS.
#include "common.h"

namespace {

constexpr int CT_W = 64, CT_H = 16;                  // classify tile: one wave per 64-pixel row segment, 4 waves x 4 rows
constexpr int TG22 = 13573;                          // int(tan(22.5 deg) * 2^15 + 0.5)
constexpr int HYST_THREADS = 1024;
constexpr size_t HYST_LDS_MAX = 147456;              // two planes of 768 x 768: 2 x 768 x 24 words
constexpr int MATCH_RMAX = 16;

DEVFN uint32_t row_mask(int W) { return (W & 31) ? ((1u << (W & 31)) - 1u) : ~0u; }     // the valid bits of a row's last word

// the two words of a wave's ballot go to words wx, wx + 1 of `row` (lanes 0 and 32 store; words at or past Wd are dropped)
DEVFN void store_ballot(uint32_t* row, int wx, int Wd, unsigned long long bal, int lane) {
    if (lane == 0 && wx < Wd) row[wx] = (uint32_t)bal;
    if (lane == 32 && wx + 1 < Wd) row[wx + 1] = (uint32_t)(bal >> 32);
}

// ---- classify: Sobel, channel choice, non-maximum suppression, two thresholds -> cand, strong ----
// LDS: the pixel tile with a halo of 2 (coordinates clamped: the replicated border), then magnitude and (dx, dy) with a halo of 1
// (magnitude 0 outside the image).  One lane per pixel; a row segment's 64 verdicts leave as one ballot.
__global__ __launch_bounds__(256) void canny_classify_kernel(const uint8_t* __restrict__ img, uint32_t* __restrict__ cand, uint32_t* __restrict__ strong,
                                                             int H, int W, int Wd, int tiles_x, int tiles_y, int low, int high) {
    __shared__ uint8_t px[3][CT_H + 4][CT_W + 4];
    __shared__ int mg[CT_H + 2][CT_W + 2];
    __shared__ int dxy[CT_H + 2][CT_W + 2];          // dx in the low half, dy in the high half (both within +-1020)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int bid = blockIdx.x;
    const int tx = bid % tiles_x;
    bid /= tiles_x;
    const int ty = bid % tiles_y, b = bid / tiles_y;
    const int x0 = tx * CT_W, y0 = ty * CT_H;
    const uint8_t* src = img + (size_t)b * H * W * 3;
    for (int i = tid; i < (CT_H + 4) * (CT_W + 4); i += 256) {
        const int py = i / (CT_W + 4), pxx = i - py * (CT_W + 4);
        const int gy = min(max(y0 - 2 + py, 0), H - 1), gx = min(max(x0 - 2 + pxx, 0), W - 1);
        const uint8_t* s = src + ((size_t)gy * W + gx) * 3;
        px[0][py][pxx] = s[0];
        px[1][py][pxx] = s[1];
        px[2][py][pxx] = s[2];
    }
    __syncthreads();
    for (int i = tid; i < (CT_H + 2) * (CT_W + 2); i += 256) {
        const int my = i / (CT_W + 2), mx = i - my * (CT_W + 2);
        const int gy = y0 - 1 + my, gx = x0 - 1 + mx;
        int m = 0, dx = 0, dy = 0;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            m = -1;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const uint8_t(*p)[CT_W + 4] = px[c];
                const int a00 = p[my][mx], a01 = p[my][mx + 1], a02 = p[my][mx + 2];
                const int a10 = p[my + 1][mx], a12 = p[my + 1][mx + 2];
                const int a20 = p[my + 2][mx], a21 = p[my + 2][mx + 1], a22 = p[my + 2][mx + 2];
                const int cdx = (a02 + 2 * a12 + a22) - (a00 + 2 * a10 + a20);
                const int cdy = (a20 + 2 * a21 + a22) - (a00 + 2 * a01 + a02);
                const int cm = abs(cdx) + abs(cdy);
                if (cm > m) { m = cm; dx = cdx; dy = cdy; }          // strictly greater: the first channel wins a tie
            }
        }
        mg[my][mx] = m;
        dxy[my][mx] = (int)(((unsigned)dy << 16) | ((unsigned)dx & 0xffffu));
    }
    __syncthreads();
    uint32_t* cplane = cand + (size_t)b * H * Wd;
    uint32_t* splane = strong + (size_t)b * H * Wd;
#pragma unroll
    for (int rr = 0; rr < CT_H / 4; rr++) {
        const int ly = wave + 4 * rr, gy = y0 + ly, gx = x0 + lane;
        const int my = ly + 1, mx = lane + 1;
        const int m = mg[my][mx], d = dxy[my][mx];
        const int dx = (int)(short)(d & 0xffff), dy = d >> 16;
        bool keep = false;
        if (gy < H && gx < W && m > low) {
            const int ax = abs(dx), ay = abs(dy) << 15, t22 = ax * TG22, t67 = t22 + (ax << 16);
            if (ay < t22) {
                keep = m > mg[my][mx - 1] && m >= mg[my][mx + 1];
            } else if (ay > t67) {
                keep = m > mg[my - 1][mx] && m >= mg[my + 1][mx];
            } else {
                const int s = ((dx ^ dy) < 0) ? -1 : 1;
                keep = m > mg[my - 1][mx - s] && m > mg[my + 1][mx + s];
            }
        }
        const unsigned long long bc = __ballot(keep), bs = __ballot(keep && m > high);
        if (gy < H) {                                 // wave-uniform
            store_ballot(cplane + (size_t)gy * Wd, x0 >> 5, Wd, bc, lane);
            store_ballot(splane + (size_t)gy * Wd, x0 >> 5, Wd, bs, lane);
        }
    }
}

// ---- pack: any channel >= t -> one bit ----
__global__ __launch_bounds__(256) void edge_pack_kernel(const uint8_t* __restrict__ img, uint32_t* __restrict__ bits, long long nseg, int W, int Wd,
                                                        int segs_x, int t) {
    const int lane = threadIdx.x & 63;
    const long long seg = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);       // wave-uniform: (image row, 64-pixel segment)
    if (seg >= nseg) return;
    const long long row = seg / segs_x;
    const int sx = (int)(seg - row * segs_x), gx = sx * 64 + lane;
    bool on = false;
    if (gx < W) {
        const uint8_t* s = img + ((size_t)row * W + gx) * 3;
        on = s[0] >= t || s[1] >= t || s[2] >= t;
    }
    store_ballot(bits + (size_t)row * Wd, sx * 2, Wd, __ballot(on), lane);
}

// ---- hysteresis: one workgroup per image, both planes in LDS ----
// g: seeds, p: where they may spread; the seeds fill their runs of p inside the word (Kogge-Stone, both directions)
DEVFN uint32_t fill_runs(uint32_t g, uint32_t p) {
    uint32_t q = p;
    g |= q & (g << 1); q &= q << 1;
    g |= q & (g << 2); q &= q << 2;
    g |= q & (g << 4); q &= q << 4;
    g |= q & (g << 8); q &= q << 8;
    g |= q & (g << 16);
    q = p;
    g |= q & (g >> 1); q &= q >> 1;
    g |= q & (g >> 2); q &= q >> 2;
    g |= q & (g >> 4); q &= q >> 4;
    g |= q & (g >> 8); q &= q >> 8;
    g |= q & (g >> 16);
    return g;
}

// Chaotic iteration of E = E | (C & dilate3x3(E)): a word may read neighbours of this round or of the last, bits are only ever set, and a
// round in which no word changed read the final state everywhere, so it ends at the least fixed point whatever the order.
__global__ __launch_bounds__(HYST_THREADS) void edge_hysteresis_kernel(const uint32_t* __restrict__ cand, const uint32_t* __restrict__ strong,
                                                                       uint32_t* __restrict__ edges, uint8_t* __restrict__ rgb,
                                                                       int* __restrict__ rounds, int H, int W, int Wd) {
    extern __shared__ __attribute__((aligned(16))) uint32_t hyst_lds[];
    const int n = H * Wd, tid = threadIdx.x;
    uint32_t* C = hyst_lds;
    uint32_t* E = hyst_lds + n;
    const size_t base = (size_t)blockIdx.x * n;
    const uint32_t last = row_mask(W);
    for (int i = tid; i < n; i += HYST_THREADS) {
        uint32_t c = cand[base + i];
        if (i % Wd == Wd - 1) c &= last;
        C[i] = c;
        E[i] = c & strong[base + i];
    }
    __syncthreads();
    const int cap = H * W + 1;
    int r = 0;
    for (;;) {
        int changed = 0;
        for (int i = tid; i < n; i += HYST_THREADS) {
            const uint32_t c = C[i], e = E[i];
            if (c == e) continue;                     // nothing left to gain here (E is a subset of C)
            const int y = i / Wd, j = i - y * Wd;
            uint32_t nb = 0;
#pragma unroll
            for (int dy = -1; dy <= 1; dy++) {
                const int yy = y + dy;
                if (yy < 0 || yy >= H) continue;
                const uint32_t* row = E + yy * Wd;
                const uint32_t v = row[j], l = j > 0 ? row[j - 1] : 0u, rt = j + 1 < Wd ? row[j + 1] : 0u;
                nb |= v | (v << 1) | (v >> 1) | (l >> 31) | (rt << 31);
            }
            const uint32_t g = e | (c & nb);
            if (g != e) {
                E[i] = fill_runs(g, c);
                changed = 1;
            }
        }
        r++;
        if (!__syncthreads_or(changed) || r >= cap) break;          // uniform: every thread sees the same OR
    }
    if (edges)
        for (int i = tid; i < n; i += HYST_THREADS) edges[base + i] = E[i];
    if (rgb) {
        const size_t nbytes = (size_t)H * W * 3;
        uint8_t* dst = rgb + (size_t)blockIdx.x * nbytes;
        auto byte_of = [&](size_t k) -> uint32_t {
            const int pix = (int)(k / 3), y = pix / W, x = pix - y * W;
            return ((E[y * Wd + (x >> 5)] >> (x & 31)) & 1u) ? 255u : 0u;
        };
        if ((((uintptr_t)rgb | nbytes) & 3) == 0) {   // every image starts on a word: four bytes per store
            uint32_t* d4 = reinterpret_cast<uint32_t*>(dst);
            for (size_t k = tid; k < nbytes / 4; k += HYST_THREADS)
                d4[k] = byte_of(4 * k) | (byte_of(4 * k + 1) << 8) | (byte_of(4 * k + 2) << 16) | (byte_of(4 * k + 3) << 24);
        } else {
            for (size_t k = tid; k < nbytes; k += HYST_THREADS) dst[k] = (uint8_t)byte_of(k);
        }
    }
    if (rounds && tid == 0) rounds[blockIdx.x] = r;
}

// ---- match counts ----
// The word (y, j) of D_r(p): the OR of rows y - r .. y + r (clipped to the image), widened to the 64 pixels around the word (16 from the
// left neighbour, 16 from the right: r <= 16), dilated r times horizontally, cut back to the word.  Padding bits are masked on every load.
DEVFN uint32_t dilated_word(const uint32_t* __restrict__ p, int y, int j, int H, int Wd, uint32_t last, int r) {
    unsigned long long t = 0;
    for (int yy = max(y - r, 0); yy <= min(y + r, H - 1); yy++) {
        const uint32_t* row = p + (size_t)yy * Wd;
        uint32_t v = row[j], l = j > 0 ? row[j - 1] : 0u, rt = j + 1 < Wd ? row[j + 1] : 0u;
        if (j == Wd - 1) v &= last;
        if (j + 1 == Wd - 1) rt &= last;
        t |= ((unsigned long long)(rt & 0xffffu) << 48) | ((unsigned long long)v << 16) | (l >> 16);
    }
    for (int s = 0; s < r; s++) t |= (t << 1) | (t >> 1);
    return (uint32_t)(t >> 16);
}

__global__ __launch_bounds__(256) void edge_match_kernel(const uint32_t* __restrict__ a, const uint32_t* __restrict__ bpl, unsigned long long* __restrict__ out,
                                                         int H, int W, int Wd, int blocks_per_image, int r) {
    __shared__ int part[4][4];
    const int img = blockIdx.x / blocks_per_image, blk = blockIdx.x - img * blocks_per_image;
    const int n = H * Wd, i = blk * 256 + threadIdx.x;
    const uint32_t* pa = a + (size_t)img * n;
    const uint32_t* pb = bpl + (size_t)img * n;
    const uint32_t last = row_mask(W);
    int cnt[4] = {0, 0, 0, 0};
    if (i < n) {
        const int y = i / Wd, j = i - y * Wd;
        const uint32_t m = j == Wd - 1 ? last : ~0u;
        const uint32_t wa = pa[i] & m, wb = pb[i] & m;
        cnt[0] = __popc(wa);
        cnt[1] = __popc(wb);
        if (wa) cnt[2] = __popc(wa & dilated_word(pb, y, j, H, Wd, last, r));
        if (wb) cnt[3] = __popc(wb & dilated_word(pa, y, j, H, Wd, last, r));
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cnt[k] += __shfl_xor(cnt[k], o, 64);
    }
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < 4; k++) part[threadIdx.x >> 6][k] = cnt[k];
    __syncthreads();
    if (threadIdx.x < 4) {
        const int s = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
        if (s) atomicAdd(out + (size_t)img * 4 + threadIdx.x, (unsigned long long)s);       // integer sums have no order
    }
}

bool image_dims_ok(int B, int H, int W) {
    return B > 0 && H > 0 && W > 0 && (unsigned long long)B * H * W * 3 < (1ull << 31);
}

}  // namespace

extern "C" {

int sidlsg_canny_classify_u8(const void* images_u8, void* cand, void* strong, int B, int H, int W, int low, int high, void* stream) {
    if (!images_u8 || !cand || !strong || !image_dims_ok(B, H, W) || low < 0 || high < low) return SIDLSG_EINVAL;
    const int Wd = (W + 31) / 32, tiles_x = (W + CT_W - 1) / CT_W, tiles_y = (H + CT_H - 1) / CT_H;
    const long long blocks = (long long)B * tiles_x * tiles_y;
    if (blocks >= (1LL << 31)) return SIDLSG_EINVAL;
    hipLaunchKernelGGL(canny_classify_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)images_u8, (uint32_t*)cand,
                       (uint32_t*)strong, H, W, Wd, tiles_x, tiles_y, low, high);
    return sidlsg_last_error();
}

int sidlsg_edge_hysteresis_lds_bytes(int H, int W) {
    if (H <= 0 || W <= 0) return SIDLSG_EINVAL;
    const unsigned long long bytes = 2ull * H * ((W + 31) / 32) * 4;
    return bytes > HYST_LDS_MAX ? SIDLSG_EINVAL : (int)bytes;
}

int sidlsg_edge_hysteresis(const void* cand, const void* strong, void* edges, void* rgb_u8, int* rounds, int B, int H, int W, void* stream) {
    if (!cand || !strong || (!edges && !rgb_u8) || !image_dims_ok(B, H, W)) return SIDLSG_EINVAL;
    const int lds = sidlsg_edge_hysteresis_lds_bytes(H, W);
    if (lds < 0) return SIDLSG_EINVAL;
    if (const int e = sidlsg_lds_limit<&edge_hysteresis_kernel>(HYST_LDS_MAX)) return e;
    hipLaunchKernelGGL(edge_hysteresis_kernel, dim3((unsigned)B), dim3(HYST_THREADS), (size_t)lds, (hipStream_t)stream, (const uint32_t*)cand,
                       (const uint32_t*)strong, (uint32_t*)edges, (uint8_t*)rgb_u8, rounds, H, W, (W + 31) / 32);
    return sidlsg_last_error();
}

int sidlsg_edge_pack_u8(const void* images_u8, void* bits, int B, int H, int W, int threshold, void* stream) {
    if (!images_u8 || !bits || !image_dims_ok(B, H, W) || threshold < 0 || threshold > 255) return SIDLSG_EINVAL;
    const int segs_x = (W + 63) / 64;
    const long long nseg = (long long)B * H * segs_x;
    hipLaunchKernelGGL(edge_pack_kernel, dim3((unsigned)((nseg + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)images_u8, (uint32_t*)bits, nseg,
                       W, (W + 31) / 32, segs_x, threshold);
    return sidlsg_last_error();
}

int sidlsg_edge_match_counts(const void* a, const void* b, void* counts, int B, int H, int W, int r, void* stream) {
    if (!a || !b || !counts || ((uintptr_t)counts & 7) || !image_dims_ok(B, H, W) || r < 0 || r > MATCH_RMAX) return SIDLSG_EINVAL;
    const int Wd = (W + 31) / 32;
    const int bpi = (int)(((long long)H * Wd + 255) / 256);
    if ((long long)B * bpi >= (1LL << 31)) return SIDLSG_EINVAL;
    if (const hipError_t e = hipMemsetAsync(counts, 0, (size_t)B * 4 * sizeof(long long), (hipStream_t)stream)) return (int)e;
    hipLaunchKernelGGL(edge_match_kernel, dim3((unsigned)((long long)B * bpi)), dim3(256), 0, (hipStream_t)stream, (const uint32_t*)a, (const uint32_t*)b,
                       (unsigned long long*)counts, H, W, Wd, bpi, r);
    return sidlsg_last_error();
}

}  // extern "C"
