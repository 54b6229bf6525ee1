// bf16 MFMA GEMM / implicit-GEMM conv3x3 for gfx950 (MI355X).
//
//   C[M,N] = epilogue( A[M,K] * W[N,K]^T )        A: dense rows or NHWC implicit im2col
//
// Covers every contraction of the SD UNet except attention:
// ResBlock conv3x3 (fwd and dgrad), 1x1 conv / Linear (fwd and dgrad), GEGLU/FF, QKV.
// Layout decisions (DESIGN.md "Data layout"): activations NHWC bf16, so a 1x1 conv and a
// Linear over tokens are the same dense GEMM; conv weights are [Cout][3][3][Cin] (K index =
// tap*Cin + c) so a K-tile of 64 lies inside one tap and an A-tile row is a contiguous
// 128-byte run of channels of one input pixel.
//
// Kernels in this file (the bf16 forward path; e4m3 operands: gemm_fp8.hip, weight gradients: wgrad.hip, what they share: gemm_core.h):
//   gemm_v3_kernel<MODE>      the main kernel (N % 160 == 0, dense rows or conv with Cin % 64 == 0, >= 384 tiles or split-K):
//                             128 x 160 x 64 tile, tiles staged by buffer_load ... lds (direct to LDS), see its header
//   gemm_bf16_kernel<BM,BN,M> every other shape (ragged N, Cin % 64 != 0, small grids): register-staged loads
//   gemm_as_kernel<NKT,RES>   A-stationary dense kernel of the wide K = 320 products (FF-in), see its header
//   gemm_p8s / gemm_p8w       the 256-row-tile kernels and their GEGLU fusions (gemm_p8.h)
//   gemm_finish_kernel        epilogue of split-K launches (fp32 slabs -> bias/residual/activation -> bf16), also for gemm_fp8.hip
// and the dispatch rules (p8_rule, dispatch_gemm) behind sidlsg_gemm_bf16*, sidlsg_gemm_geglu*, sidlsg_conv3x3_bf16* and sidlsg_conv3x3_br_bf16.
// Common tiling: 256 threads = 4 waves (2x2); block tile BM x BN x 64, wave tile 64 x BN/2 as 16x16x32 MFMAs; LDS double
// buffer, 128-byte rows with a 16-byte-chunk XOR swizzle that makes every ds_read_b128 lane group conflict free.
// Loads are branch-free: every operand is read through a buffer resource with the hardware range check -- an
// out-of-image tap / row >= M / k >= K lane simply gets the OOB offset and reads zeros.  Row offsets are computed once
// per tap (a wave-uniform event every Cin/64 tiles).  The MFMA is issued "transposed" (rows = output channel, cols =
// pixel) and W-tile rows are permuted per tile pair so that each lane ends up with 8 consecutive output channels of one
// pixel: the epilogue stores 16 bytes per lane.
#include "gemm_core.h"

#ifdef SIDLSG_EXP_TRACE           // measurement build: one call arms (or, with null, disarms) the phase timestamps of this unit and of wgrad.hip
extern "C" int sidlsg_exp_set_trace(void* ptr) { return exp_set_trace_here(ptr) | sidlsg_exp_set_trace_wgrad(ptr); }
#endif

// PAD (conv modes): rows / columns of zero padding in front of the image, 1 = torch's padding=1; 0 = the window of output (i, j) starts at
// input (stride i, stride j) and only its far side can leave the image (sidlsg_conv3x3_br_bf16: padding on the bottom and right only).
template <int BM, int BN, int MODE, int PAD = 1>
__global__ __launch_bounds__(NTHREADS, 2) void gemm_bf16_kernel(GemmParams p) {   // 2 blocks/CU: <= 256 registers
    constexpr int WMT = BM / 2, WNT = BN / 2;   // wave tile
    constexpr int MT = WMT / 16, NT = WNT / 16;
    constexpr int AR = BM / 32, BR = BN / 32;   // 16B chunks per thread per tile
    extern __shared__ __attribute__((aligned(16))) char smem[];
    bf16* As = reinterpret_cast<bf16*>(smem);                 // [2][BM][BK]
    bf16* Bs = As + 2 * BM * BK;                              // [2][BN][BK]

    // ---- XCD-aware block -> tile map: blocks that share an A row-panel sit on one XCD (own L2)
    const int tiles_n = (p.N + BN - 1) / BN;
    const int tiles_m = m_tiles_rt(p, BM);
    const int nblk = tiles_n * tiles_m;
    const int bid = xcd_contiguous((int)blockIdx.x, nblk);
    const int m0 = group_select<BM>(p, bid / tiles_n);
    const int n0 = (bid % tiles_n) * BN;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm0 = (wave >> 1) * WMT, wn0 = (wave & 1) * WNT;
    const int kc = tid & 7, r0 = tid >> 3;

    const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16*>(p.A), 0, (int)p.a_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16*>(p.W), 0, (int)p.w_bytes, 0x00020000);

    // ---- per-thread row descriptors (byte offsets; OOB = reads zeros)
    const int Hs = p.ups ? (p.H >> 1) : p.H, Ws = p.ups ? (p.Wd >> 1) : p.Wd;
    unsigned abase[AR];      // dense: row offset (+ chunk); conv: batch image offset (+ chunk)
    int ahi[AR], awi[AR];    // conv: top-left input coordinate of the 3x3 window
    unsigned arow[AR];       // conv MODE 1: current per-tap row offset
#pragma unroll
    for (int i = 0; i < AR; i++) {
        const int m = m0 + r0 + 32 * i;
        const bool ok = m < p.M;
        if (MODE == 0) {
            abase[i] = ok ? (unsigned)m * (unsigned)p.lda * 2u + kc * 16u : OOB;
            ahi[i] = awi[i] = 0;
        } else {
            const ConvRow cr = conv_row(p, m);
            abase[i] = (unsigned)cr.b * (unsigned)(Hs * Ws) * (unsigned)p.lda * 2u + kc * 16u;
            ahi[i] = cr.hi(p, PAD);
            awi[i] = cr.wi(p, PAD);
        }
        arow[i] = OOB;
    }
    unsigned bbase[BR];
#pragma unroll
    for (int i = 0; i < BR; i++) {
        const int n = n0 + r0 + 32 * i;
        bbase[i] = n < p.N ? (unsigned)n * (unsigned)p.K * 2u + kc * 16u : OOB;
    }

    auto tap_rows = [&](int tap) {   // MODE 1: wave-uniform tap -> per-row offsets
        const int dh = tap / 3, dw = tap - dh * 3;
#pragma unroll
        for (int i = 0; i < AR; i++) {
            int hi = ahi[i] + dh, wi = awi[i] + dw;
            const bool ok = hi >= 0 && hi < p.H && wi >= 0 && wi < p.Wd;
            if (p.ups) { hi >>= 1; wi >>= 1; }
            arow[i] = ok ? abase[i] + (unsigned)(hi * Ws + wi) * (unsigned)p.lda * 2u : OOB;
        }
    };

    bf16x8 areg[AR], breg[BR];
    int cur_tap = -1;
    auto load_tile = [&](int kt) {
        const int k0 = kt * BK;
        const bool kok = k0 + kc * 8 < p.K;
        if (MODE == 0) {
#pragma unroll
            for (int i = 0; i < AR; i++) areg[i] = buf_ld8(ra, kok ? abase[i] + (unsigned)k0 * 2u : OOB);
        } else if (MODE == 1) {
            const int tap = k0 / p.Cin;          // scalar
            const int c0 = k0 - tap * p.Cin;
            if (tap != cur_tap) { tap_rows(tap); cur_tap = tap; }
#pragma unroll
            for (int i = 0; i < AR; i++) areg[i] = buf_ld8(ra, arow[i] + (unsigned)c0 * 2u);
        } else {
            const int k = k0 + kc * 8;
            const int tap = k / p.Cin, c = k - tap * p.Cin;
            const int dh = tap / 3, dw = tap - dh * 3;
#pragma unroll
            for (int i = 0; i < AR; i++) {
                int hi = ahi[i] + dh, wi = awi[i] + dw;
                const bool ok = kok && hi >= 0 && hi < p.H && wi >= 0 && wi < p.Wd;
                if (p.ups) { hi >>= 1; wi >>= 1; }
                // abase already contains kc*16 bytes; replace it by the channel offset of this chunk
                areg[i] = buf_ld8(ra, ok ? abase[i] - kc * 16u + ((unsigned)(hi * Ws + wi) * (unsigned)p.lda + (unsigned)c) * 2u : OOB);
            }
        }
#pragma unroll
        for (int i = 0; i < BR; i++) breg[i] = buf_ld8(rw, kok ? bbase[i] + (unsigned)k0 * 2u : OOB);
    };
    auto store_tile = [&](int buf) {
        bf16* a = As + buf * BM * BK;
        bf16* b = Bs + buf * BN * BK;
#pragma unroll
        for (int i = 0; i < AR; i++) {
            const int r = r0 + 32 * i;
            st8(a + r * BK + ((kc ^ ((r >> 1) & 7)) << 3), areg[i]);
        }
#pragma unroll
        for (int i = 0; i < BR; i++) {
            const int r = r0 + 32 * i;
            st8(b + r * BK + ((kc ^ ((r >> 1) & 7)) << 3), breg[i]);
        }
    };

    f32x4 acc[NT][MT];
#pragma unroll
    for (int i = 0; i < NT; i++)
#pragma unroll
        for (int j = 0; j < MT; j++) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // operand row (within the wave's n range) that lane (l&15) of n-tile ni supplies
    const int li = lane & 15, lg = lane >> 4;
    int wrow[NT];
#pragma unroll
    for (int ni = 0; ni < NT; ni++) {
        const bool paired = (ni | 1) < NT;
        wrow[ni] = wn0 + (paired ? 32 * (ni >> 1) + (li >> 2) * 8 + (ni & 1) * 4 + (li & 3) : 16 * ni + li);
    }

    const int nk_all = (p.K + BK - 1) / BK;
    const int kt_begin = p.kt_per_split ? blockIdx.y * p.kt_per_split : 0;
    const int nk = p.kt_per_split ? min(nk_all, kt_begin + p.kt_per_split) : nk_all;

    auto read_frags = [&](int buf, int kk, bf16x8 (&fa)[MT], bf16x8 (&fw)[NT]) {
        const bf16* a = As + buf * BM * BK;
        const bf16* b = Bs + buf * BN * BK;
        const int ch = kk * 4 + lg;
#pragma unroll
        for (int mi = 0; mi < MT; mi++) {
            const int r = wm0 + mi * 16 + li;
            fa[mi] = *reinterpret_cast<const bf16x8*>(a + r * BK + ((ch ^ ((r >> 1) & 7)) << 3));
        }
#pragma unroll
        for (int ni = 0; ni < NT; ni++) {
            const int r = wrow[ni];
            fw[ni] = *reinterpret_cast<const bf16x8*>(b + r * BK + ((ch ^ ((r >> 1) & 7)) << 3));
        }
    };
    auto mfma_block = [&](const bf16x8 (&fa)[MT], const bf16x8 (&fw)[NT]) {
#pragma unroll
        for (int ni = 0; ni < NT; ni++)
#pragma unroll
            for (int mi = 0; mi < MT; mi++)
                acc[ni][mi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fw[ni], fa[mi], acc[ni][mi], 0, 0, 0);
    };

    // Software pipeline (one barrier per K-tile, no exposed LDS latency):
    //   A: issue the kk=1 fragment reads of the current LDS buffer, run the kk=0 MFMAs on the fragments prefetched earlier
    //   B: commit the staged next tile (global -> registers, in flight since the previous D) to the other LDS buffer
    //   C: barrier   (the current buffer is now fully in registers, the next one fully written)
    //   D: issue the kk=0 fragment reads of the NEXT buffer and the global loads of the tile after it
    //   E: run the kk=1 MFMAs, which cover the latencies of D
    bf16x8 fa0[MT], fw0[NT], fa1[MT], fw1[NT];
    load_tile(kt_begin);
    store_tile(0);
    __syncthreads();
    read_frags(0, 0, fa0, fw0);
    if (kt_begin + 1 < nk) load_tile(kt_begin + 1);
    auto ktile = [&](const int kt, auto has_next, auto fetch) {     // straight-line instantiations: see gemm_v3_kernel
        const int buf = (kt - kt_begin) & 1;
        read_frags(buf, 1, fa1, fw1);          // A
        mfma_block(fa0, fw0);
        if constexpr (decltype(has_next)::value) store_tile(buf ^ 1);         // B
        __syncthreads();                       // C
        if constexpr (decltype(has_next)::value) {                            // D
            read_frags(buf ^ 1, 0, fa0, fw0);
            if constexpr (decltype(fetch)::value) load_tile(kt + 2);
        }
        mfma_block(fa1, fw1);                  // E
    };
    {
        int kt = kt_begin;
        for (; kt + 2 < nk; kt++) ktile(kt, std::true_type{}, std::true_type{});
        if (kt + 1 < nk) { ktile(kt, std::true_type{}, std::false_type{}); kt++; }
        ktile(kt, std::false_type{}, std::false_type{});
    }

    if (p.kt_per_split) {
        // split-K: raw fp32 partial sums into the workspace; gemm_finish_kernel applies the epilogue
#pragma unroll
        for (int mi = 0; mi < MT; mi++) {
            const int m = m0 + wm0 + mi * 16 + li;
            if (m >= p.M) continue;
#pragma unroll
            for (int ni = 0; ni < NT; ni++) {
                const bool paired = (ni | 1) < NT;
                const int nb = n0 + wn0 + (paired ? 32 * (ni >> 1) + lg * 8 + (ni & 1) * 4 : 16 * ni + lg * 4);
                float* dst = p.ws + ((size_t)blockIdx.y * p.Mtot + m) * p.N + nb;     // this split's slab: plain 16-byte stores
                if (nb + 4 <= p.N) *reinterpret_cast<f32x4*>(dst) = acc[ni][mi];
                else
                    for (int r = 0; r < 4; r++)
                        if (nb + r < p.N) dst[r] = acc[ni][mi][r];
            }
        }
        return;
    }
    EpiPre<NT> pre;
    epilogue_prefetch<NT>(p, pre, n0 + wn0, lg);
    gemm_epilogue<MT, NT>(p, acc, m0 + wm0, n0 + wn0, li, lg, pre);
}

// epilogue of a split-K GEMM: C = act(alpha * sum_s slab_s + bias + rowvec + res)
__global__ void gemm_finish_kernel(GemmParams p, int nsp) {      // nsp: number of K splits (slabs)
    const size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i >= (size_t)p.M * p.N) return;
    const int m = (int)(i / p.N), n = (int)(i - (size_t)m * p.N);      // N % 4 == 0 on this path
    const size_t slab = (size_t)p.M * p.N;
    f32x4 v = *reinterpret_cast<const f32x4*>(p.ws + i);
    int sidx = 1;
    for (; sidx + 3 < nsp; sidx += 4) {                   // four independent loads in flight, fixed summation order
        const f32x4 a = *reinterpret_cast<const f32x4*>(p.ws + (size_t)sidx * slab + i);
        const f32x4 b = *reinterpret_cast<const f32x4*>(p.ws + (size_t)(sidx + 1) * slab + i);
        const f32x4 c = *reinterpret_cast<const f32x4*>(p.ws + (size_t)(sidx + 2) * slab + i);
        const f32x4 d = *reinterpret_cast<const f32x4*>(p.ws + (size_t)(sidx + 3) * slab + i);
        v += a; v += b; v += c; v += d;
    }
    for (; sidx < nsp; sidx++) v += *reinterpret_cast<const f32x4*>(p.ws + sidx * slab + i);
    const float* rv = p.rowvec ? p.rowvec + (size_t)(m / p.rows_per_batch) * p.ldrv : nullptr;
    const float* bias = (p.Mg && m >= p.Mg) ? p.bias1 : p.bias;      // grouped launch: the row's set
#pragma unroll
    for (int e = 0; e < 4; e++) {
        float x = v[e] * p.alpha;
        if (bias) x += bias[n + e];
        if (rv) x += rv[n + e];
        if (p.res) x += bf2f(p.res[(size_t)m * p.ldres + n + e]);
        if (p.flags & F_SILU) x = silu_f(x);
        v[e] = x;
    }
    if (p.flags & F_OUT_F32) {
        float* c = reinterpret_cast<float*>(p.C) + (size_t)m * p.ldc + n;
        if (p.flags & F_ACCUM) { for (int e = 0; e < 4; e++) c[e] += v[e]; }
        else *reinterpret_cast<f32x4*>(c) = v;
    } else {
        bf16x4 o = {f2bf(v[0]), f2bf(v[1]), f2bf(v[2]), f2bf(v[3])};
        *reinterpret_cast<bf16x4*>(reinterpret_cast<bf16*>(p.C) + (size_t)m * p.ldc + n) = o;
    }
}

// Second launch of a split-K GEMM: the `splits` slabs of p.ws -> C through the epilogue (gemm_finish_kernel, four outputs per thread).
// External linkage: the mx8 launcher of gemm_fp8.hip splits K too.  (The caller has put SIDLSG_FIN_GEMM into its dispatch record.)
void launch_gemm_finish(const GemmParams& p, int splits, hipStream_t s) {
    const size_t n4 = ((size_t)p.M * p.N + 3) / 4;
    SIDLSG_LAUNCH(gemm_finish_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, p, splits);
}

// ---------------------------------------------------------------------------------------------
// "v3": the 128 x 160 x 64 tile / 4 waves / 2 blocks per CU structure of gemm_bf16_kernel, but tiles are staged by
// direct-to-LDS loads (global_load_lds_dwordx4 + zero page, source-side swizzle as in v2): the ds_write commit phase --
// measured at ~25 % of the kernel and not overlapped with MFMA -- and the staging registers disappear.
// Schedule per K-tile (2 LDS buffers, one raw barrier):
//   A: issue the kk=1 fragment reads of the current buffer; kk=0 MFMAs (fragments were prefetched in the previous D)
//   C: s_waitcnt vmcnt(0) (this wave's DMA of tile kt+1 has landed) ; s_barrier
//   D: issue the kk=0 fragment reads of tile kt+1 and the DMA of tile kt+2 into the buffer just vacated
//   E: kk=1 MFMAs (cover D's latencies)
// (A 3-buffer ring with counted vmcnt(9) -- every DMA gets two K-tiles of MFMA time, but 108 KiB of LDS = ONE block per CU
// -- was measured in the same session: 30-50 % SLOWER on every SD shape (e.g. conv 64x64 320->320 124 -> 195 us, FF-in 239 ->
// 355 us).  Two co-resident blocks per CU hide more than a deeper pipeline in one; the variant is not in the build.)
template <int MODE, int STAGES>   // MODE 0 dense, 1 conv3x3 with Cin % 64 == 0
DEVFN void gemm_v3_body(GemmParams& p) {
    constexpr int BM = 128, BN = 160, MT = 4, NT = 5;
    constexpr bool SCHED_FENCE = SIDLSG_V3_SCHED_FENCE;
    constexpr int STAGE = (BM + BN) * BK;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    bf16* ring = reinterpret_cast<bf16*>(smem);

    // Work item = (output tile, K split), 1-D grid.  Hardware block b runs on XCD b % 8; the remap gives every XCD a
    // contiguous range of logical items.  Logical order: split-major, and inside a split the tiles in groups of 8
    // m-tiles (m fastest, then n): the ~64 blocks resident on an XCD then form an ~8 x 8 patch of output tiles and
    // fetch 8 A panels + 8 W panels into that XCD's L2.  (Row-major strips fetched 1 A panel + 64 W panels for FF-in
    // at 16x16 -- every XCD streamed the whole weight matrix; measured 154 -> 130 us on 4096x10240x1280 and 90 -> 72
    // us on the 8x8 2560->1280 conv.)
    const int tiles_n = (p.N + BN - 1) / BN;
    const int tiles_m = m_tiles_rt(p, BM);
#ifdef SIDLSG_EXP_K1             // measurement build: one K-tile per output tile (prologue + epilogue cost)
    const int nk_all = 1;
#else
    const int nk_all = (p.K + BK - 1) / BK;
#endif
    const int nsplit = p.kt_per_split ? (nk_all + p.kt_per_split - 1) / p.kt_per_split : 1;
    const int ntile = tiles_n * tiles_m;
    const int bid = xcd_contiguous((int)blockIdx.x, ntile * nsplit);
    const int split = bid / ntile;
    int mt, nt;
    {
        const int t = bid - split * ntile;
        const int per_group = p.group_m * tiles_n;
        const int g = t / per_group, first_m = g * p.group_m;
        const int gm = min(p.group_m, tiles_m - first_m);       // last group may be short
        const int in_g = t - g * per_group;
        mt = first_m + in_g % gm;
        nt = in_g / gm;
    }
    const int m0 = group_select<BM>(p, mt);
    const int n0 = nt * BN;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm0 = (wave >> 1) * 64, wn0 = (wave & 1) * 80;
    const int li = lane & 15, lg = lane >> 4;
    const int lrow = lane >> 3, lslot = lane & 7;

    // first output column of this wave's half of the tile (fused GEGLU: the a half / the gate half live F columns apart)
    const int wcol0 = p.geglu ? (wn0 ? p.geglu + nt * 80 : nt * 80) : n0 + wn0;

    // Loader: buffer_load_dwordx4 ... lds.  Per row ONE 32-bit byte offset (VGPR) that already contains the lane's
    // swizzled chunk; the K position of the tile is the wave-uniform soffset.  Invalid rows (m >= M, n >= N, conv halo)
    // carry an out-of-range offset and the buffer unit writes zeros: no pointer arithmetic, selects or zero page in the
    // steady state (the 64-bit global_load_lds version issued ~150 VALU+SALU per 40 MFMAs).
    const int Hs = p.ups ? (p.H >> 1) : p.H, Ws = p.ups ? (p.Wd >> 1) : p.Wd;
    // conv, K-tile order "channel chunk outer, tap inner" (`lin`): the 9 taps of a chunk re-read the same 3 image rows shifted
    // by a pixel; visited back to back the re-reads hit the XCD's L2 (FETCH_SIZE 291 -> 123 MB per launch at 64x64x320 -> 320,
    // 713 -> 143 MB at 640 channels; with the tap-major order the reuse distance was Cin * 256 B = 80-330 KB per block, times
    // ~64 resident blocks per XCD = 5-20 MB against 4 MB of L2).  The weight matrix stays tap-major, only the visiting order
    // changes.  Addressing: the byte offset of tap (dh, dw) is LINEAR in (dh, dw) with wave-uniform strides, so the per-row
    // VGPR holds the CENTRE pixel's offset, the tap goes into the scalar soffset (against a buffer base moved one row + one
    // pixel below A, so soffset >= 0), and the halo is a 9-bit validity mask per row: 3 VALU per row and K-tile instead of a
    // recomputation of the row offsets (which cost 5 % when done per K-tile).  Not with the fused nearest x2 upsampling
    // ((h + dh) >> 1 is not linear): that keeps the tap-major order.
    const unsigned tap_rs = (unsigned)Ws * (unsigned)p.lda * 2u, tap_ps = (unsigned)p.lda * 2u;
    const bool lin = MODE == 1 && SIDLSG_CONV_TAP_INNER && !p.ups && (unsigned long long)p.a_bytes + tap_rs + tap_ps < 0x80000000ull;
    const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<bf16*>(p.A) - (lin ? (size_t)(tap_rs + tap_ps) / 2 : 0), 0, (int)(p.a_bytes + (lin ? tap_rs + tap_ps : 0u)), 0x00020000);
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16*>(p.W), 0, (int)p.w_bytes, 0x00020000);
    unsigned abase[4], aoff[4];
    int ahi[4], awi[4];
    unsigned cen[4], tmask[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int r = wave * 32 + j * 8 + lrow;
        const int kcs = lslot ^ ((r >> 1) & 7);
        const int m = m0 + r;
        const bool ok = m < p.M;
        if (MODE == 0) {
            aoff[j] = ok ? ((unsigned)m * (unsigned)p.lda + kcs * 8) * 2u : OOB;
            abase[j] = 0; ahi[j] = awi[j] = 0;
        } else {
            const ConvRow cr = conv_row(p, m);
            abase[j] = ((unsigned)(cr.b * Hs * Ws) * (unsigned)p.lda + kcs * 8) * 2u;
            ahi[j] = cr.hi(p, 1);
            awi[j] = cr.wi(p, 1);
            aoff[j] = OOB;
            cen[j] = abase[j] + (unsigned)((ahi[j] + 1) * Ws + awi[j] + 1) * tap_ps;
            unsigned mk = 0;
#pragma unroll
            for (int tp = 0; tp < 9; tp++) {
                const int hi = ahi[j] + tp / 3, wi = awi[j] + tp % 3;
                if (hi >= 0 && hi < p.H && wi >= 0 && wi < p.Wd) mk |= 1u << tp;
            }
            tmask[j] = mk;
        }
    }
    if (MODE == 0) {
#pragma unroll
        for (int j = 0; j < 4; j++) cen[j] = tmask[j] = 0;
    }
    unsigned boff[5];
#pragma unroll
    for (int j = 0; j < 5; j++) {
        const int g = wave + 4 * j;                 // 20 groups of 8 weight rows, 5 per wave
        const int r = g * 8 + lrow;
        const int kcs = lslot ^ wsw(r);
        const int n = p.geglu ? (r < 80 ? nt * 80 + r : p.geglu + nt * 80 + (r - 80)) : n0 + r;      // fused GEGLU: a rows | gate rows
        boff[j] = n < p.N ? ((unsigned)n * (unsigned)p.K + kcs * 8) * 2u : OOB;
    }
    const int kt_begin = p.kt_per_split ? split * p.kt_per_split : 0;
    const int nk = p.kt_per_split ? min(nk_all, kt_begin + p.kt_per_split) : nk_all;
    int cur_tap = -1;

    auto issue = [&](int t, int buf) {          // 9 buffer_load ... lds per wave
        bf16* sa = ring + buf * STAGE;
        bf16* sb = sa + BM * BK;
        int k0 = t * BK;
        int asoff = k0 * 2;
        if (MODE == 1) {
            if (lin) {
                const int cc = t / 9;
                const int tap = t - cc * 9;
                const int dh = tap / 3, dw = tap - dh * 3;
                asoff = cc * BK * 2 + dh * (int)tap_rs + dw * (int)tap_ps;
                k0 = tap * p.Cin + cc * BK;
                const unsigned bit = 1u << tap;
#pragma unroll
                for (int j = 0; j < 4; j++) aoff[j] = (tmask[j] & bit) ? cen[j] : OOB;
                cur_tap = tap;
            }
            const int tap = lin ? cur_tap : k0 / p.Cin;
            if (!lin) asoff = (k0 - tap * p.Cin) * 2;
            if (tap != cur_tap) {               // every Cin/64 tiles: new tap -> new row offsets / halo mask
                cur_tap = tap;
                const int dh = tap / 3, dw = tap - dh * 3;
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    int hi = ahi[j] + dh, wi = awi[j] + dw;
                    const bool v = hi >= 0 && hi < p.H && wi >= 0 && wi < p.Wd;
                    if (p.ups) { hi >>= 1; wi >>= 1; }
                    aoff[j] = v ? abase[j] + (unsigned)(hi * Ws + wi) * (unsigned)p.lda * 2u : OOB;
                }
            }
        }
        if (MODE == 0 && k0 + BK > p.K) {       // ragged K tail (dense only): chunks past K must read zeros
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int r = wave * 32 + j * 8 + lrow;
                const int kcs = lslot ^ ((r >> 1) & 7);
                const unsigned o = (k0 + kcs * 8 < p.K) ? aoff[j] : OOB;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (lptr_t)(sa + (wave * 32 + j * 8) * BK), 16, o, asoff, 0, 0);
            }
#pragma unroll
            for (int j = 0; j < 5; j++) {
                const int g = wave + 4 * j;
                const int kcs = lslot ^ wsw(g * 8 + lrow);
                const unsigned o = (k0 + kcs * 8 < p.K) ? boff[j] : OOB;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (lptr_t)(sb + g * 8 * BK), 16, o, k0 * 2, 0, 0);
            }
            return;
        }
#pragma unroll
        for (int j = 0; j < 4; j++)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (lptr_t)(sa + (wave * 32 + j * 8) * BK), 16, aoff[j], asoff, 0, 0);
#pragma unroll
        for (int j = 0; j < 5; j++)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (lptr_t)(sb + (wave + 4 * j) * 8 * BK), 16, boff[j], k0 * 2, 0, 0);
    };

    f32x4 acc[NT][MT];
#pragma unroll
    for (int i = 0; i < NT; i++)
#pragma unroll
        for (int j = 0; j < MT; j++) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    int wrow[NT];
#pragma unroll
    for (int ni = 0; ni < NT; ni++) {
        const bool paired = (ni | 1) < NT;
        wrow[ni] = wn0 + (paired ? 32 * (ni >> 1) + (li >> 2) * 8 + (ni & 1) * 4 + (li & 3) : 16 * ni + li);
    }
    auto read_frags = [&](int buf, int kk, bf16x8 (&fa)[MT], bf16x8 (&fw)[NT]) {
        const bf16* a = ring + buf * STAGE;
        const bf16* b = a + BM * BK;
        const int ch = kk * 4 + lg;
#pragma unroll
        for (int mi = 0; mi < MT; mi++) {
            const int r = wm0 + mi * 16 + li;
            fa[mi] = *reinterpret_cast<const bf16x8*>(a + r * BK + ((ch ^ ((r >> 1) & 7)) << 3));
        }
#pragma unroll
        for (int ni = 0; ni < NT; ni++) {
            const int r = wrow[ni];
            fw[ni] = *reinterpret_cast<const bf16x8*>(b + r * BK + ((ch ^ wsw(r)) << 3));
        }
    };
    auto mfma_block = [&](const bf16x8 (&fa)[MT], const bf16x8 (&fw)[NT]) {
        if constexpr ((SIDLSG_V3_PRIO) & 1) V3_SETPRIO(1);
#pragma unroll
        for (int ni = 0; ni < NT; ni++)
#pragma unroll
            for (int mi = 0; mi < MT; mi++)
                acc[ni][mi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fw[ni], fa[mi], acc[ni][mi], 0, 0, 0);
        if constexpr ((SIDLSG_V3_PRIO) & 1) V3_SETPRIO(0);
    };

    bf16x8 fa0[MT], fw0[NT], fa1[MT], fw1[NT];
    EpiPre<NT> pre;
    if constexpr (STAGES == 2) {
    TRACE(0); TRACE_HWID();
    issue(kt_begin, 0);
    if (!p.kt_per_split) epilogue_prefetch<NT>(p, pre, wcol0, lg);        // behind the first tile's DMA, used after the loop
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    TRACE(1);
    read_frags(0, 0, fa0, fw0);
#ifdef SIDLSG_EXP_NOLDS
    read_frags(0, 1, fa1, fw1);
#endif
    if (kt_begin + 1 < nk) issue(kt_begin + 1, 1);
    // One K-tile.  The steady state, the last-but-one tile (nothing left to fetch) and the last tile are separate
    // STRAIGHT-LINE instantiations: with `if (more)` / `if (kt + 2 < nk)` inside one loop body the waitcnt pass has to merge
    // the paths and makes the kk=1 MFMAs of E wait for the fragment reads D has just issued (lgkmcnt(4..0) in the ISA instead
    // of ~9), i.e. the prefetch of the next tile's fragments was serialised in front of the MFMAs meant to cover it.
    auto ktile = [&](const int kt, auto has_next, auto fetch) {
        const int buf = (kt - kt_begin) & 1;
#ifndef SIDLSG_EXP_NOLDS
        read_frags(buf, 1, fa1, fw1);                          // A
#endif
        mfma_block(fa0, fw0);
        // The MFMAs are register-only, so neither the "memory" clobber nor the barrier orders them: without this fence the
        // scheduler hoists the wait + barrier to right behind the FIRST kk=0 MFMA (seen in the ISA), which halves the MFMA
        // time covering the DMA of tile kt+1 (issued in the previous D) and serialises the wait in front of 19 MFMAs.
        if (SCHED_FENCE) __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // C: my share of tile kt+1 is in LDS
#ifndef SIDLSG_EXP_NOBAR
        __builtin_amdgcn_s_barrier();
#endif
        asm volatile("" ::: "memory");
        if (SCHED_FENCE) __builtin_amdgcn_sched_barrier(0);
        if constexpr (decltype(has_next)::value) {             // D
#ifndef SIDLSG_EXP_NOLDS
            read_frags(buf ^ 1, 0, fa0, fw0);
#endif
#ifndef SIDLSG_EXP_NODMA
            if constexpr (decltype(fetch)::value) issue(kt + 2, buf);
#endif
        }
        mfma_block(fa1, fw1);                                  // E
    };
    {
        int kt = kt_begin;
        for (; kt + 2 < nk; kt++) ktile(kt, std::true_type{}, std::true_type{});
        if (kt + 1 < nk) { ktile(kt, std::true_type{}, std::false_type{}); kt++; }
        ktile(kt, std::false_type{}, std::false_type{});
    }

    }

    if (p.kt_per_split) {
#pragma unroll
        for (int mi = 0; mi < MT; mi++) {
            const int m = m0 + wm0 + mi * 16 + li;
            if (m >= p.M) continue;
#pragma unroll
            for (int ni = 0; ni < NT; ni++) {
                const bool paired = (ni | 1) < NT;
                const int nb = n0 + wn0 + (paired ? 32 * (ni >> 1) + lg * 8 + (ni & 1) * 4 : 16 * ni + lg * 4);
                float* dst = p.ws + ((size_t)split * p.Mtot + m) * p.N + nb;
                if (nb + 4 <= p.N) *reinterpret_cast<f32x4*>(dst) = acc[ni][mi];
                else
                    for (int r = 0; r < 4; r++)
                        if (nb + r < p.N) dst[r] = acc[ni][mi][r];
            }
        }
        return;
    }
#ifndef SIDLSG_EXP_DIRECT_STORE
    if (!(p.flags & (F_OUT_F32 | F_ACCUM)) && (p.N & 7) == 0) {
        constexpr int LDR = BN + 8;             // 336-byte rows: the 16 rows of a b128 write phase fall on distinct banks
        __syncthreads();                        // every wave is done with the last K-tile: the ring becomes the tile image
        TRACE(2);
        gemm_epilogue<MT, NT>(p, acc, m0 + wm0, wcol0, li, lg, pre, ring, m0, wcol0 - wn0, LDR);
        __syncthreads();
        TRACE(3);
        if (MODE == 0 && p.geglu) {       // (dense kernel only: the conv instantiation does not carry this code)
            // the staged tile holds h[.., 0:80) = a and h[.., 80:160) = gate of features [80 nt, +80): write both (natural
            // columns; skipped when the caller keeps no h: a pass without backward) and y = a * gelu(gate) -- from the bf16-ROUNDED
            // values, i.e. bit for bit what sidlsg_geglu_fwd computes from the stored h
            constexpr int CPR = 10;                 // 16-byte chunks of the 80 features
            bf16* H = reinterpret_cast<bf16*>(p.C);
#pragma unroll
            for (int i = 0; i < (BM * CPR + NTHREADS - 1) / NTHREADS; i++) {
                const int c = tid + i * NTHREADS;
                const int row = c / CPR, col = (c - row * CPR) * 8;
                const int m = m0 + row;
                if (row < BM && m < p.M) {
                    const bf16x8 av = *reinterpret_cast<const bf16x8*>(ring + row * LDR + col);
                    const bf16x8 gv = *reinterpret_cast<const bf16x8*>(ring + row * LDR + 80 + col);
                    const int f = nt * 80 + col;
                    if (H) {
                        st8(H + (size_t)m * p.ldc + f, av);
                        st8(H + (size_t)m * p.ldc + p.geglu + f, gv);
                    }
                    bf16x8 o;
#pragma unroll
                    for (int e = 0; e < 8; e++) o[e] = f2bf(bf2f(av[e]) * gelu_t<bf16>(bf2f(gv[e])));
                    st8(p.Y + (size_t)m * p.ldy + f, o);
                }
            }
            return;
        }
#ifndef SIDLSG_EXP_NO_GEGLU_BWD       // (measurement build: the kernel without this epilogue, to price its code size)
        if (MODE == 0 && p.geglu_bwd) {       // (dense kernel only)
            // the staged tile holds the bf16-ROUNDED dy of 160 features: bit for bit what sidlsg_geglu_bwd computes from a stored dy.
            // Every h load of a half is issued before that half's first store (Hin / dH do not alias: __restrict__ locals).
            constexpr int CPR = BN / 8;                             // 16-byte chunks per tile row
            constexpr int ITER = BM * CPR / NTHREADS / 2;           // chunks per thread and half
            static_assert(BM * CPR % (2 * NTHREADS) == 0, "whole passes");
            const int F = p.geglu_bwd;
            const bf16* __restrict__ Hin = p.Hin;
            bf16* __restrict__ dH = p.Y;
#pragma unroll
            for (int half = 0; half < 2; half++) {
                bf16x8 av[ITER], gv[ITER];
#pragma unroll
                for (int i = 0; i < ITER; i++) {
                    const int c = tid + (half * ITER + i) * NTHREADS;
                    const int row = c / CPR, col = (c - row * CPR) * 8;
                    const bool ok = m0 + row < p.M && n0 + col < p.N;
                    const size_t o = (size_t)(m0 + row) * p.ldy + n0 + col;
                    av[i] = ok ? ld8(Hin + o) : zero8();
                    gv[i] = ok ? ld8(Hin + o + F) : zero8();
                }
#pragma unroll
                for (int i = 0; i < ITER; i++) {
                    const int c = tid + (half * ITER + i) * NTHREADS;
                    const int row = c / CPR, col = (c - row * CPR) * 8;
                    if (!(m0 + row < p.M && n0 + col < p.N)) continue;
                    const bf16x8 dv = *reinterpret_cast<const bf16x8*>(ring + row * LDR + col);
                    bf16x8 da, dg;
#pragma unroll
                    for (int e = 0; e < 8; e++) {
                        float gl, gd;
                        gelu_pair_t<bf16>(bf2f(gv[i][e]), gl, gd);
                        const float d = bf2f(dv[e]);
                        da[e] = f2bf(d * gl);
                        dg[e] = f2bf(d * bf2f(av[i][e]) * gd);
                    }
                    const size_t o = (size_t)(m0 + row) * p.ldy + n0 + col;
                    st8(dH + o, da);
                    st8(dH + o + F, dg);
                }
            }
            return;
        }
#endif
        gemm_store_rows<BM, BN>(p, ring, m0, n0, LDR, tid);
        TRACE(4);
#ifdef SIDLSG_EXP_TRACE
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        TRACE(5);
#endif
        return;
    }
    gemm_epilogue<MT, NT, false>(p, acc, m0 + wm0, n0 + wn0, li, lg, pre);
#else
    gemm_epilogue<MT, NT>(p, acc, m0 + wm0, n0 + wn0, li, lg, pre);
#endif
}

// (plain kernels over one body: a kernel template with a second non-type parameter got no host stub from hipcc 7.2)
template <int MODE>
__global__ __launch_bounds__(NTHREADS, 2) void gemm_v3_kernel(GemmParams p) { gemm_v3_body<MODE, 2>(p); }

template <int MODE>
static int launch_gemm_v3(const GemmParams& p, hipStream_t s) {
    const int tiles = m_tiles_rt(p, 128) * ((p.N + 159) / 160);
    const size_t lds = (size_t)2 * (128 + 160) * BK * sizeof(bf16);
    const int nk = (p.K + BK - 1) / BK;
    const int splits = p.kt_per_split ? (nk + p.kt_per_split - 1) / p.kt_per_split : 1;
    GemmParams q = p;
    static const int group_env = sidlsg_env_int("SIDLSG_GEMM_GROUP_M", 4);   // A/B switch (measured: 4 and 8 equivalent, 1 = row-major strips)
    q.group_m = group_env < 1 ? 1 : group_env;
    record_launch(SIDLSG_K_GEMM_V3, 128, 160, MODE, -1, -1, splits, p.kt_per_split ? SIDLSG_PART_SLABS : SIDLSG_PART_ONE);
    if (p.kt_per_split) record_followup(SIDLSG_FIN_GEMM);
    if (const int e = sidlsg_lds_limit<&gemm_v3_kernel<MODE>>(lds)) return e;
    SIDLSG_LAUNCH((gemm_v3_kernel<MODE>), dim3(tiles * splits), dim3(NTHREADS), lds, s, q);
    if (p.kt_per_split) launch_gemm_finish(p, splits, s);
    return sidlsg_last_error();
}

#include "gemm_p8.h"

// ---------------------------------------------------------------------------------------------------------------------
// "A-stationary" dense GEMM for the wide short-contraction products of the 64 x 64 stage (K = 320, N >= 2560: the FF-in
// projection).  The shape is memory bound (65536 x 2560 x 320: 42 MB in, 335 MB out, 107 GFLOP = 63 us of HBM time against
// 43 us of MFMA time) and ran at a third of either bound in gemm_v3_kernel: with 5 K-tiles per output tile a block spends as
// long in its prologue (first tile DMA: nothing to overlap it), epilogue and store drain as in the K loop, and every K-tile
// waits a full L2 -> LDS round trip because only one tile is in flight.
// Here a block keeps its 128 x 320 panel of A in LDS for its whole life (80 KiB, loaded once) and walks over the 160-wide
// column tiles of its range; the W tiles stream through a 3-slot ring as ONE continuous sequence of 160 x 64 chunks -- the
// DMA of chunk s+3 is issued when chunk s has been read, so two chunks are always in flight and no tile restarts the
// pipeline -- the epilogue's loads (bias, residual) are issued at the tile's first chunk, and its stores drain behind the
// next tile's MFMAs.  That needs counted waits, which works because EVERY vector-memory operation of the loop is a buffer
// operation that is always issued (out-of-range lanes carry the OOB offset instead of being predicated off): the
// s_waitcnt vmcnt(N) immediates below count them exactly.  One block of 4 waves per CU (LDS: 80 + 60 + 10 KiB).
// Output tile -> global memory through a per-wave 16 x 80 LDS transposition buffer (row-major 160-byte runs; the MFMA
// layout's 64-byte half lines are taken at half rate by the L2, see gemm_store_rows).
// Measured (MI355X, in-session A/B against gemm_v3_kernel): 65536 x 2560 x 320 220 -> 157 us, 32768 x 2560 x 320 86 -> 77 us;
// N = 1280 / 960 tie and N = 320 loses (two tiles do not amortise the panel load with one block per CU) -> dispatched from
// N = 2560.  Variants measured slower and not kept: 8 waves with 32 x 80 wave tiles (1.55x the LDS fragment traffic per MFMA:
// 172 us), and the write-out software-pipelined into the next tile's chunks (its LDS round trips stall the MFMA stream: 185 us).
// Requires K == 64 * NKT, N % 160 == 0, bf16 output, no row vector / activation / fp32 / accumulate flags.
struct AsLoads {          // epilogue operands of one tile, fetched at its first chunk
    f32x4 b[5];
    bf16x8 r[4][3];
};
template <int NKT, bool RES>
__global__ __launch_bounds__(NTHREADS, 1) void gemm_as_kernel(GemmParams p) {
    constexpr int BM = 128, BN = 160, MT = 4, NT = 5, R = 3;
    constexpr int ACH = BM * BK, WST = BN * BK, LDT = 80;
    constexpr int NLD = 5 + (RES ? 12 : 0);     // buffer loads of AsLoads per wave
    constexpr int NST = 12;                      // buffer stores of one tile's epilogue per wave
    extern __shared__ __attribute__((aligned(16))) char smem[];
    bf16* Ap = reinterpret_cast<bf16*>(smem);    // [NKT][128][64]
    bf16* Wr = Ap + NKT * ACH;                   // [R][160][64]
    bf16* Tb = Wr + R * WST;                     // [4 waves][16][LDT]
    const int tiles_n = p.N / BN;
    const int tpi = p.group_m;                   // column tiles per work item
    const int items_per_panel = (tiles_n + tpi - 1) / tpi;
    const int bid = xcd_contiguous((int)blockIdx.x, (int)gridDim.x);
    const int mt = bid / items_per_panel, it = bid - mt * items_per_panel;
    const int m0 = group_select<BM>(p, mt);
    const int nt0 = it * tpi, ntl = min(tpi, tiles_n - nt0);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm0 = (wave >> 1) * 64, wn0 = (wave & 1) * 80;
    const int li = lane & 15, lg = lane >> 4;
    const int lrow = lane >> 3, lslot = lane & 7;
    const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16*>(p.A), 0, (int)p.a_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16*>(p.W), 0, (int)p.w_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.bias), 0, p.bias ? p.N * 4 : 0, 0x00020000);
    const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16*>(p.res), 0, 0x7FFFFFFF, 0x00020000);
    const __amdgpu_buffer_rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<bf16*>(p.C), 0, 0x7FFFFFFF, 0x00020000);

    // ---- A panel: all NKT chunks at once (4 DMAs per wave and chunk)
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int r = wave * 32 + j * 8 + lrow;
        const int kcs = lslot ^ ((r >> 1) & 7);
        const int m = m0 + r;
        const unsigned off = m < p.M ? ((unsigned)m * (unsigned)p.lda + kcs * 8) * 2u : OOB;
#pragma unroll
        for (int kc = 0; kc < NKT; kc++)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (lptr_t)(Ap + kc * ACH + (wave * 32 + j * 8) * BK), 16, off, kc * BK * 2, 0, 0);
    }
    // ---- W stream: chunk s = (tile s / NKT of this item, K chunk s % NKT) -> ring slot s % R
    unsigned boff[5];
#pragma unroll
    for (int j = 0; j < 5; j++) {
        const int r = (wave + 4 * j) * 8 + lrow;
        boff[j] = ((unsigned)r * (unsigned)p.K + (lslot ^ wsw(r)) * 8) * 2u;
    }
    const int S = ntl * NKT;
    // (every lambda of this kernel is force-inlined: a closure left out of line drags the kernel arguments into scratch and
    // the buffer descriptors into VGPRs -> waterfall loops around every buffer operation)
    auto issue_w = [&](int s2) __attribute__((always_inline)) {   // always 5 DMAs; past the end of the item they fetch nothing (zeros into a dead slot)
        const int t = s2 / NKT, kc = s2 - t * NKT;
        const int slot = s2 % R;
        const unsigned so = ((unsigned)((nt0 + t) * BN) * (unsigned)p.K + kc * BK) * 2u;
        const bool live = s2 < S;
#pragma unroll
        for (int j = 0; j < 5; j++)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (lptr_t)(Wr + slot * WST + (wave + 4 * j) * 8 * BK), 16, live ? boff[j] : OOB, live ? so : 0u, 0, 0);
    };
    issue_w(0); issue_w(1); issue_w(2);

    f32x4 acc[NT][MT];
    int wrow[NT];
#pragma unroll
    for (int ni = 0; ni < NT; ni++) {
        const bool paired = (ni | 1) < NT;
        wrow[ni] = wn0 + (paired ? 32 * (ni >> 1) + (li >> 2) * 8 + (ni & 1) * 4 + (li & 3) : 16 * ni + li);
    }
    auto read_frags = [&](int kc, int slot, int kk, bf16x8 (&fa)[MT], bf16x8 (&fw)[NT]) __attribute__((always_inline)) {
        const bf16* a = Ap + kc * ACH;
        const bf16* b = Wr + slot * WST;
        const int ch = kk * 4 + lg;
#pragma unroll
        for (int mi = 0; mi < MT; mi++) {
            const int r = wm0 + mi * 16 + li;
            fa[mi] = *reinterpret_cast<const bf16x8*>(a + r * BK + ((ch ^ ((r >> 1) & 7)) << 3));
        }
#pragma unroll
        for (int ni = 0; ni < NT; ni++) {
            const int r = wrow[ni];
            fw[ni] = *reinterpret_cast<const bf16x8*>(b + r * BK + ((ch ^ wsw(r)) << 3));
        }
    };
    auto mfma_block = [&](const bf16x8 (&fa)[MT], const bf16x8 (&fw)[NT]) __attribute__((always_inline)) {
#pragma unroll
        for (int ni = 0; ni < NT; ni++)
#pragma unroll
            for (int mi = 0; mi < MT; mi++)
                acc[ni][mi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fw[ni], fa[mi], acc[ni][mi], 0, 0, 0);
    };
    // epilogue operands of the tile whose first column is n0: 5 bias loads (+ 12 residual loads), always issued
    auto tile_loads = [&](int n0, AsLoads& L) __attribute__((always_inline)) {
        const int nb = n0 + wn0;
        L.b[0] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rb, (unsigned)(nb + lg * 8) * 4u, 0, 0));
        L.b[1] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rb, (unsigned)(nb + lg * 8 + 4) * 4u, 0, 0));
        L.b[2] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rb, (unsigned)(nb + 32 + lg * 8) * 4u, 0, 0));
        L.b[3] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rb, (unsigned)(nb + 32 + lg * 8 + 4) * 4u, 0, 0));
        L.b[4] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rb, (unsigned)(nb + 64 + lg * 4) * 4u, 0, 0));
        if (RES) {
#pragma unroll
            for (int mi = 0; mi < MT; mi++) {
                const int m = m0 + wm0 + mi * 16 + li;
                const bool ok = m < p.M;
                const unsigned row = ok ? (unsigned)m * (unsigned)p.ldres : 0u;
#pragma unroll
                for (int pr = 0; pr < 3; pr++) {
                    const int n = nb + 32 * pr + lg * (pr < 2 ? 8 : 4);
                    const unsigned off = ok ? (row + (unsigned)n) * 2u : OOB;
                    if (pr < 2) L.r[mi][pr] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rr, off, 0, 0));
                    else {
                        const u32x2 t = __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(rr, off, 0, 0));
                        L.r[mi][pr] = __builtin_bit_cast(bf16x8, (u32x4){t[0], t[1], 0u, 0u});
                    }
                }
            }
        }
    };
    // acc -> bf16 tile -> global: per 16-row block through this wave's LDS buffer, 3 buffer stores (160-byte rows)
    bf16* tb = Tb + wave * 16 * LDT;
    auto epilogue = [&](int n0, const AsLoads& L) __attribute__((always_inline)) {
#pragma unroll
        for (int mi = 0; mi < MT; mi++) {
#pragma unroll
            for (int pr = 0; pr < 3; pr++) {
                float v[8];
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    v[r] = acc[2 * pr][mi][r] * p.alpha + L.b[pr < 2 ? 2 * pr : 4][r];
                    v[4 + r] = pr < 2 ? acc[pr < 2 ? 2 * pr + 1 : 0][mi][r] * p.alpha + L.b[pr < 2 ? 2 * pr + 1 : 0][r] : 0.f;
                }
                if (RES) {
#pragma unroll
                    for (int e = 0; e < (pr < 2 ? 8 : 4); e++) v[e] += bf2f(L.r[mi][pr][e]);
                }
                if (pr < 2) {
                    bf16x8 o;
#pragma unroll
                    for (int e = 0; e < 8; e++) o[e] = f2bf(v[e]);
                    st8(tb + li * LDT + 32 * pr + lg * 8, o);
                } else {
                    bf16x4 o = {f2bf(v[0]), f2bf(v[1]), f2bf(v[2]), f2bf(v[3])};
                    *reinterpret_cast<bf16x4*>(tb + li * LDT + 64 + lg * 4) = o;
                }
            }
            // wave-private buffer: the LDS counter orders the writes above before the reads below (and the reads before
            // the next block's writes)
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const int c = lane + 64 * j;                    // 16 rows x 10 chunks of 16 bytes
                const int row = c / 10, col = (c - row * 10) * 8;
                const int m = m0 + wm0 + mi * 16 + row;
                const bool ok = c < 160 && m < p.M;
                const bf16x8 val = *reinterpret_cast<const bf16x8*>(tb + (c < 160 ? row * LDT + col : 0));
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, val), rc,
                                                       ok ? ((unsigned)m * (unsigned)p.ldc + (unsigned)(n0 + wn0 + col)) * 2u : OOB, 0, 0);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
#pragma unroll
        for (int i = 0; i < NT; i++)
#pragma unroll
            for (int j = 0; j < MT; j++) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    };

#pragma unroll
    for (int i = 0; i < NT; i++)
#pragma unroll
        for (int j = 0; j < MT; j++) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    bf16x8 fa0[MT], fw0[NT], fa1[MT], fw1[NT];
    // the A panel and chunk 0 have landed when at most chunks 1 and 2 (10 DMAs) are outstanding
    asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    read_frags(0, 0, 0, fa0, fw0);

    // One W chunk (step s = t * NKT + kc).  WAIT = number of vector-memory operations issued AFTER the DMAs of chunk s+1
    // at the point of the wait: chunk s+1 has landed when no more than that many are outstanding.
    auto step = [&](const int s, const int kc, auto wait_c) __attribute__((always_inline)) {
        constexpr int WAIT = decltype(wait_c)::value;
        const int slot = s % R;
        read_frags(kc, slot, 1, fa1, fw1);
        mfma_block(fa0, fw0);
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(WAIT) : "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        read_frags(kc + 1 == NKT ? 0 : kc + 1, (s + 1) % R, 0, fa0, fw0);     // chunk s+1 (a dead read after the last step)
        issue_w(s + 3);                                                         // into the slot chunk s just vacated
        mfma_block(fa1, fw1);
    };
    // Outstanding operations younger than chunk s+1's DMAs at the wait of step (t, kc) -- program order per tile:
    //   [tile loads NLD] step 0 .. step NKT-1, each ending with 5 DMAs, [epilogue stores NST]
    //   kc = 0: chunk s+2 (5, issued in the previous tile's last step) + previous epilogue's NST stores + this tile's NLD loads
    //   kc = 1: previous stores + loads + chunk s+2 (5, issued in step 0)     kc >= 2: chunk s+2 only
    // first tile of the item: no previous epilogue (kc = 0: chunk 2 + loads; kc = 1: loads + chunk 3)
    using std::integral_constant;
    AsLoads L;
    auto tile = [&](const int t, auto first) __attribute__((always_inline)) {
        constexpr bool FIRST = decltype(first)::value;
        const int n0 = (nt0 + t) * BN;
        tile_loads(n0, L);
        const int s0 = t * NKT;
        step(s0, 0, integral_constant<int, 5 + NLD + (FIRST ? 0 : NST)>{});
        if constexpr (NKT > 1) step(s0 + 1, 1, integral_constant<int, 5 + NLD + (FIRST ? 0 : NST)>{});
#pragma unroll
        for (int kc = 2; kc < NKT; kc++) step(s0 + kc, kc, integral_constant<int, 5>{});
        epilogue(n0, L);
    };
    tile(0, std::true_type{});
    for (int t = 1; t < ntl; t++) tile(t, std::false_type{});
}

template <int NKT>
static int launch_gemm_as(const GemmParams& p, hipStream_t s) {
    constexpr size_t lds = (size_t)(NKT * 128 * BK + 3 * 160 * BK + 4 * 16 * 80) * sizeof(bf16);
    const int panels = m_tiles_rt(p, 128), tiles_n = p.N / 160;
    // work item = (panel, range of column tiles): whole panels when they fill the chip, else split the column range so that
    // ~512 items exist (an item re-loads its A panel: keep ranges >= 2 tiles when N allows)
    int tpi = tiles_n;
    while (tpi > 2 && (long long)panels * ((tiles_n + tpi - 1) / tpi) < 512) tpi = (tpi + 1) / 2;
    GemmParams q = p;
    q.group_m = tpi;
    const int items = panels * ((tiles_n + tpi - 1) / tpi);
    record_launch(SIDLSG_K_GEMM_AS, 128, 160, 0, -1, -1, 1, SIDLSG_PART_ONE);
    if (const int e = p.res ? sidlsg_lds_limit<&gemm_as_kernel<NKT, true>>(lds) : sidlsg_lds_limit<&gemm_as_kernel<NKT, false>>(lds)) return e;
    if (p.res) SIDLSG_LAUNCH((gemm_as_kernel<NKT, true>), dim3(items), dim3(NTHREADS), lds, s, q);
    else SIDLSG_LAUNCH((gemm_as_kernel<NKT, false>), dim3(items), dim3(NTHREADS), lds, s, q);
    return sidlsg_last_error();
}

// (A multi-stage variant of the 64 x 64 fallback below -- "s64": buffer_load ... lds into a 4-slot ring, three K-tiles in flight, counted
// vmcnt waits, the v3 fragment layout -- was built in round 5 on the theory that the ~250 small launches per iteration (text K / V
// projections, 8 x 8 stage Linears: 17 - 20 us each in the step's profile) are bound by one L2 -> LDS round trip per K-tile.  Measured
// alone (tools/ab/small_gemm.py under rocprofv3) they are not: 1232 x 640 x 768 7.4 us with either kernel, 1024 x 1280 x 1280 12.9 ->
// 11.2, 2048 x 1280 x 1280 17.2 -> 18.7, step 209.98 vs 209.87 ms -- their time in the step is chip sharing, not their own latency.
// Correct (the shapes are in tests/test_gpu_ops.py::test_gemm), neutral, not in the build: commit "gemm_s64_kernel" of round 5.)
template <int BM, int BN, int MODE, int PAD = 1>
static int launch_gemm(const GemmParams& p, hipStream_t s) {
    const int tiles = m_tiles_rt(p, BM) * ((p.N + BN - 1) / BN);
    const size_t lds = (size_t)2 * (BM + BN) * BK * sizeof(bf16);
    const int nk = (p.K + BK - 1) / BK;
    const int splits = p.kt_per_split ? (nk + p.kt_per_split - 1) / p.kt_per_split : 1;
    record_launch(SIDLSG_K_GEMM_BF16, BM, BN, MODE, PAD, -1, splits, p.kt_per_split ? SIDLSG_PART_SLABS : SIDLSG_PART_ONE);
    if (p.kt_per_split) record_followup(SIDLSG_FIN_GEMM);
    if (const int e = sidlsg_lds_limit<&gemm_bf16_kernel<BM, BN, MODE, PAD>>(lds)) return e;
    SIDLSG_LAUNCH((gemm_bf16_kernel<BM, BN, MODE, PAD>), dim3(tiles, splits), dim3(NTHREADS), lds, s, p);
    if (p.kt_per_split) launch_gemm_finish(p, splits, s);
    return sidlsg_last_error();
}

// Which p8 configuration a call takes when nothing forces one (-1: none, the v3 / bf16 kernels), and with how many K splits.
// A small cost model with constants measured by tools/ubench/p8_bench on MI355X (profiles/r06_p8_ab.txt), microseconds:
//   v3  (128 x 160 tiles, 512 resident):  rounds * (11  + 1.03 * k-tiles per split)
//   p8W (256 x 320 tiles, 256 resident):  rounds * (16  + 1.61 * k-tiles per split)      13 with slab stores instead of the epilogue
//   p8S (256 x 160 tiles, 256 resident):  rounds * (8.5 + 1.03 * k-tiles per split)       7
//   split-K adds the slab round trip + gemm_finish_kernel: (8 * splits + 4) * M * N bytes at ~10 TB/s (the slabs stay in the Infinity Cache)
// i.e. the W tile's K loop runs at 1.67 PFLOP/s against 1.30 (half the staged bytes and 0.7x the fragment reads per MFMA); its
// blocks all finish at the same time (residual reads + output writes of the entire launch with no MFMA work beside them), which
// the row-major epilogue of gemm_p8.h keeps at the HBM time of those bytes.  The S tile has v3's bytes per MFMA and v3's K loop; what
// it saves is epilogue time per output byte -- worth 8-10 % stand-alone on the short-K dense GEMMs (K = 320 ... 640: five to ten
// K-tiles per tile), nothing on the convolutions (+-3 %), and nothing in the step (201.7 vs 201.8 ms per iteration with / without it,
// profiles/r06_p8_step_ab.txt): the rule offers it to dense calls only and only with SIDLSG_P8_S=1.
struct P8Choice { int cfg, splits; };
template <int MODE>
static P8Choice p8_rule(const GemmParams& p, const Ws& w) {
    static const int margin_pct = sidlsg_env_int("SIDLSG_P8_MARGIN", 3);
    static const bool dense_too = sidlsg_env_on("SIDLSG_P8_DENSE");      // A/B switch: dense GEMMs by the same model
    static const bool s_too = sidlsg_env_int("SIDLSG_P8_S", 0) != 0;                     // A/B switch: the 256 x 160 configuration for dense GEMMs (off: neutral in the step)
    if ((MODE == 0 && !dense_too) || p.N % 160 || p.K % BK || p.M <= 0) return {-1, 1};      // (nothing below divides by a zero tile count)
    const int nk = p.K / BK;
    const double mn = (double)p.M * p.N;
    auto fin = [&](int s) { return s > 1 ? (8.0 * s + 4.0) * mn / 10e6 : 0.0; };
    const long long cap = w.ptr && w.bytes > 0 ? w.bytes / (long long)(mn * 4) : 1;
    // v3 as dispatch_gemm would launch it: the same split-K rule with the same knobs
    const long long t3 = (long long)m_tiles_rt(p, 128) * (p.N / 160);
    const int s3 = splitk_splits_bf16(t3, nk, (long long)p.M * p.N, w);
    const double v3_us = (double)((t3 * s3 + 511) / 512) * (11.0 + 1.03 * ((nk + s3 - 1) / s3)) + fin(s3);
    P8Choice best{-1, 1};
    double best_us = v3_us * 100.0 / (100 + margin_pct);
    for (int cfg = 1; cfg >= 0; cfg--) {
        if ((cfg == 0 && (MODE != 0 || !s_too)) || !p8_ok<MODE>(p, cfg)) continue;
        const long long t = (long long)m_tiles_rt(p, 256) * (p.N / (cfg ? 320 : 160));
        const double f1 = cfg ? 16.0 : 8.5, fs = cfg ? 13.0 : 7.0, slope = cfg ? 1.61 : 1.03;
        for (int s = 1; s <= 8; s++) {
            if (s > 1 && (s > cap || nk / s < 12 || (t * s > 256 && t * (s - 1) >= 256))) break;
            const double us = (double)((t * s + 255) / 256) * ((s > 1 ? fs : f1) + slope * ((nk + s - 1) / s)) + fin(s);
            if (us < best_us) { best_us = us; best = {cfg, s}; }
        }
    }
    return best;
}

template <int MODE>
static int dispatch_gemm(const GemmParams& pin, hipStream_t s) {
    GemmParams p = pin;
    p.Mtot = p.M;
    // algorithmic bytes: A read once (conv: the image, not its 9-fold im2col), W once per weight set, C written once, + the residual
    const double a_elems = MODE == 0 ? (double)p.M * p.K : (double)p.M / (p.Ho * p.Wo) * (p.ups ? (p.H / 2) * (p.Wd / 2) : p.H * p.Wd) * p.Cin;
    SidlsgTraceScope ts(MODE == 0 ? SIDLSG_FAM_GEMM : SIDLSG_FAM_CONV, 2.0 * p.M * (double)p.N * p.K,
                        2.0 * (a_elems + (double)p.N * p.K * (p.Mg ? 2 : 1) + (double)p.M * p.N * ((p.flags & F_OUT_F32) ? 2 : 1) + (p.res ? (double)p.M * p.N : 0.0)));
    // N multiple of 160 (every SD channel count is a multiple of 320) -> exact 160-wide tiles and, for dense rows /
    // Cin % 64 == 0 convs, the direct-to-LDS kernel (v3); otherwise 128-wide; narrow outputs (conv_out, dgrad of conv_in)
    // -> 64-wide.  Small pixel counts (8x8 / 16x16 stages, small batches) would give < 256 tiles = idle CUs: split K when
    // the contraction is long, else fall back to 64-row and then 64x64 tiles until the grid covers the chip.
    if (p.N <= 64) return launch_gemm<128, 64, MODE>(p, s);
    if constexpr (MODE == 0) {
        static const bool as_on = sidlsg_env_on("SIDLSG_GEMM_AS");   // A/B switch
        static const int as_min_n = sidlsg_env_int("SIDLSG_GEMM_AS_MIN_N", 2560);   // measured break-even
        if (as_on && p.K == 320 && p.N % 160 == 0 && p.N >= as_min_n && p.M >= 8192 && !p.rowvec && !p.flags && !p.kt_per_split && (p.ldc & 7) == 0 &&
            (!p.res || (p.ldres & 7) == 0) && (long long)p.M * p.ldc < (1ll << 30) && (!p.res || (long long)p.M * p.ldres < (1ll << 30)))
            return launch_gemm_as<5>(p, s);
    }
    auto tiles = [&](int bm, int bn) { return (long long)m_tiles_rt(p, bm) * ((p.N + bn - 1) / bn); };
    // p8 kernels (gemm_p8.h): 256-row tiles, one block per CU.  g_p8_mode: -1 = by rule, 0 = never, 1 / 2 = always the S / W
    // configuration when the call is admissible (A/B switch: SIDLSG_GEMM_P8, sidlsg_debug_set_p8)
    if constexpr (MODE != 2) {
        const int mode = p8_mode();
        const Ws w = ws_for(s);
        const int nk = p.K / BK;
        P8Choice ch{-1, 1};
        if (mode == 1 || mode == 2) {           // forced configuration: split K towards one block per CU
            ch.cfg = p8_ok<MODE>(p, mode - 1) ? mode - 1 : -1;
            const long long t = tiles(256, ch.cfg == 1 ? 320 : 160);
            if (ch.cfg >= 0 && t < 192 && w.ptr && (long long)p.M * p.N * 8 <= w.bytes)
                ch.splits = std::max(1, (int)std::min<long long>(std::min<long long>((256 + t - 1) / t, w.bytes / ((long long)p.M * p.N * 4)), std::min(nk / 12, 16)));
        } else if (mode < 0) {
            ch = p8_rule<MODE>(p, w);
        }
        if (ch.cfg >= 0) {
            GemmParams q = p;
            if (ch.splits >= 2) { q.kt_per_split = (nk + ch.splits - 1) / ch.splits; q.ws = w.ptr; }
            return ch.cfg ? launch_gemm_p8<MODE == 2 ? 0 : MODE, 1>(q, s) : launch_gemm_p8<MODE == 2 ? 0 : MODE, 0>(q, s);
        }
    }
    const bool n160 = p.N % 160 == 0;
    static const bool v3_on = sidlsg_env_on("SIDLSG_GEMM_V3");   // A/B switch
    const bool v3 = n160 && v3_on && MODE != 2;
    static const int V3_DIRECT_TILES = sidlsg_env_int("SIDLSG_V3_DIRECT_TILES", 256);   // 256 since the compact epilogue: 4096x1280x1280 28.1 -> 23.9 us
    if ((p.N & 3) == 0) {              // (gemm_finish_kernel handles four columns per thread)
        const int nk = (p.K + BK - 1) / BK;
        const Ws w = ws_for(s);
        const int splits = splitk_splits_bf16(tiles(128, n160 ? 160 : 128), nk, (long long)p.M * p.N, w);
        if (splits >= 2) {
            GemmParams q = p;
            q.kt_per_split = (nk + splits - 1) / splits;
            q.ws = w.ptr;
            if (v3) return launch_gemm_v3<MODE == 2 ? 0 : MODE>(q, s);
            return n160 ? launch_gemm<128, 160, MODE>(q, s) : launch_gemm<128, 128, MODE>(q, s);
        }
    }
    if (tiles(128, n160 ? 160 : 128) >= (v3 ? V3_DIRECT_TILES : 384)) {
        if (v3) return launch_gemm_v3<MODE == 2 ? 0 : MODE>(p, s);
        return n160 ? launch_gemm<128, 160, MODE>(p, s) : launch_gemm<128, 128, MODE>(p, s);
    }
    if (tiles(64, n160 ? 160 : 128) >= 384) return n160 ? launch_gemm<64, 160, MODE>(p, s) : launch_gemm<64, 128, MODE>(p, s);
    return launch_gemm<64, 64, MODE>(p, s);
}

extern "C" {

// Dense GEMM: C[M,N] = act(alpha * A[M,K] W[N,K]^T + bias[N] + rowvec[m/rpb,N] + res[M,N])
static int gemm_bf16_impl(bool g2, const void* A, int lda, const void* W, const void* W1, void* C, int ldc, const float* bias, const float* bias1,
                          const void* res, int ldres, const float* rowvec, int ld_rowvec, int rows_per_batch, int M, int N, int K, float alpha,
                          int flags, void* stream) {
    if (g2 && !group2_args_ok(M, W1, bias, bias1)) return SIDLSG_EINVAL;
    GemmParams p = dense_params(A, lda, W, C, ldc, bias, res, ldres, rowvec, ld_rowvec, rows_per_batch, M, N, K, alpha, flags);
    if (int e = check_common(p)) return e;
    if (!range31(p.a_bytes, M, lda, K, 2) || !range31(p.w_bytes, N, K, K, 2)) return SIDLSG_EINVAL;
    set_group2(p, g2, W1, nullptr, bias1);
    if (int e = check_epilogue(p)) return e;
    return dispatch_gemm<0>(p, (hipStream_t)stream);
}
int sidlsg_gemm_bf16(const void* A, int lda, const void* W, void* C, int ldc, const float* bias, const void* res,
                     int ldres, const float* rowvec, int ld_rowvec, int rows_per_batch, int M, int N, int K, float alpha,
                     int flags, void* stream) {
    return gemm_bf16_impl(false, A, lda, W, nullptr, C, ldc, bias, nullptr, res, ldres, rowvec, ld_rowvec, rows_per_batch, M, N, K, alpha, flags, stream);
}

// Grouped dense GEMM: two weight sets on one stacked activation matrix (M even): rows [0, M/2) use (W, bias), rows [M/2, M)
// use (W1, bias1); res / rowvec / C are stacked like A.  One launch fills the chip where each half alone would not (the frozen
// fake-score and teacher passes of phase B read identical inputs: sid_training_loop.py:494-506).  bf16 only.
int sidlsg_gemm_bf16_g2(const void* A, int lda, const void* W, const void* W1, void* C, int ldc, const float* bias, const float* bias1,
                        const void* res, int ldres, const float* rowvec, int ld_rowvec, int rows_per_batch, int M, int N, int K,
                        float alpha, int flags, void* stream) {
    return gemm_bf16_impl(true, A, lda, W, W1, C, ldc, bias, bias1, res, ldres, rowvec, ld_rowvec, rows_per_batch, M, N, K, alpha, flags, stream);
}

// FF-in projection + GEGLU in one kernel: h[M][N2] = A W^T + bias (N2 = 2 F; H may be NULL: not stored),
// Y[M][F] = h[:, :F] * gelu(h[:, F:]).  Runs on the direct-to-LDS kernel only: returns SIDLSG_EINVAL for shapes it would not take
// (F % 80, K % 64, fewer output tiles than the kernel is dispatched for) -- sidlsg_gemm_geglu_ok tells beforehand.
int sidlsg_gemm_geglu_ok(int M, int N2, int K) {
    static const bool on = sidlsg_env_on("SIDLSG_GEMM_GEGLU");      // A/B switch
    if (!on || M <= 0 || N2 <= 0 || K <= 0 || (N2 % 160) || (K & 7)) return 0;
    return (long long)((M + 127) / 128) * (N2 / 160) >= 256 ? 1 : 0;
}
// (the two fusions go straight to their kernels: no dispatch_gemm, no check_common; g2: the grouped forms below)
static int gemm_geglu_impl(bool g2, const void* A, int lda, const void* W, const void* W1, void* H, int ldh, void* Y, int ldy, const float* bias,
                           const float* bias1, int M, int N2, int K, void* stream) {
    if (!sidlsg_gemm_geglu_ok(M, N2, K) || !A || !W || !Y || (ldy & 7) || (ldh & 7) || (lda & 7)) return SIDLSG_EINVAL;
    if (g2 && !group2_args_ok(M, W1, bias, bias1)) return SIDLSG_EINVAL;
    GemmParams p = dense_params(A, lda, W, H, ldh, bias, nullptr, 0, nullptr, N2, 1, M, N2, K, 1.f, 0);
    p.Y = (bf16*)Y; p.ldy = ldy; p.geglu = N2 / 2; p.Mtot = M;
    if (!range31(p.a_bytes, M, lda, K, 2) || !range31(p.w_bytes, N2, K, K, 2)) return SIDLSG_EINVAL;
    set_group2(p, g2, W1, nullptr, bias1);
    SidlsgTraceScope ts(SIDLSG_FAM_GEMM, 2.0 * M * (double)N2 * K,
                        2.0 * ((double)M * K + (g2 ? 2.0 : 1.0) * (double)N2 * K + (double)M * N2 * (H ? 1.5 : 0.5)));
    if (p8_geglu_takes(p)) return launch_gemm_p8_geglu<1>(p, (hipStream_t)stream);
    return launch_gemm_v3<0>(p, (hipStream_t)stream);
}
int sidlsg_gemm_geglu_bf16(const void* A, int lda, const void* W, void* H, int ldh, void* Y, int ldy, const float* bias, int M, int N2,
                           int K, void* stream) {
    return gemm_geglu_impl(false, A, lda, W, nullptr, H, ldh, Y, ldy, bias, nullptr, M, N2, K, stream);
}

// Data gradient of the FF-out projection + GEGLU derivative in one kernel: dy = dOut Wt^T (Wt = the [F][K] backward-data operand of
// the [K][F] FF-out weight; dy [M][F] is never stored), dH[:, :F] = dy * gelu(h[:, F:]), dH[:, F:] = dy * h[:, :F] * gelu'(h[:, F:]).
// Direct-to-LDS kernel only, same admission rule as the forward fusion.
int sidlsg_gemm_geglu_bwd_ok(int M, int F, int K) {
    static const bool on = sidlsg_env_on("SIDLSG_GEMM_GEGLU_BWD");      // A/B switch
#ifdef SIDLSG_EXP_NO_GEGLU_BWD
    return 0;
#endif
    if (!on || M <= 0 || F <= 0 || K <= 0 || (F % 160) || (K & 7)) return 0;
    return (long long)((M + 127) / 128) * (F / 160) >= 256 ? 1 : 0;
}
static int gemm_geglu_bwd_impl(bool g2, const void* dOut, int lda, const void* Wt, const void* Wt1, const void* H, void* dH, int ldh, int M, int F,
                               int K, void* stream) {
    if (!sidlsg_gemm_geglu_bwd_ok(M, F, K) || !dOut || !Wt || !H || !dH || (ldh & 7) || (lda & 7) || ldh < 2 * F) return SIDLSG_EINVAL;
    if (g2 && !group2_args_ok(M, Wt1, nullptr, nullptr)) return SIDLSG_EINVAL;
    GemmParams p = dense_params(dOut, lda, Wt, nullptr, F, nullptr, nullptr, 0, nullptr, F, 1, M, F, K, 1.f, 0);      // dy is never stored: no C
    p.Y = (bf16*)dH; p.Hin = (const bf16*)H; p.ldy = ldh; p.geglu_bwd = F; p.Mtot = M;
    if (!range31(p.a_bytes, M, lda, K, 2) || !range31(p.w_bytes, F, K, K, 2)) return SIDLSG_EINVAL;
    set_group2(p, g2, Wt1, nullptr, nullptr);
    SidlsgTraceScope ts(SIDLSG_FAM_GEMM, 2.0 * M * (double)F * K, 2.0 * ((double)M * K + (g2 ? 2.0 : 1.0) * (double)F * K + 4.0 * (double)M * F));
    if (p8_geglu_takes(p)) return launch_gemm_p8_geglu<2>(p, (hipStream_t)stream);
    return launch_gemm_v3<0>(p, (hipStream_t)stream);
}
int sidlsg_gemm_geglu_bwd_bf16(const void* dOut, int lda, const void* Wt, const void* H, void* dH, int ldh, int M, int F, int K,
                               void* stream) {
    return gemm_geglu_bwd_impl(false, dOut, lda, Wt, nullptr, H, dH, ldh, M, F, K, stream);
}

// Grouped variants of the two GEGLU fusions (round 6: the grouped frozen pass of phase B -- 64 of an iteration's 144 sample-passes -- had fallen back
// to the unfused chain: grouped FF-in GEMM, stand-alone GEGLU, grouped FF-out dgrad, stand-alone GEGLU backward).  Rows [0, M/2) use (W, bias) / Wt,
// rows [M/2, M) use (W1, bias1) / Wt1; everything else as in the single-set entry points (group_select narrows each block to its set, the epilogues
// only see the block's rows).
int sidlsg_gemm_geglu_bf16_g2(const void* A, int lda, const void* W, const void* W1, void* H, int ldh, void* Y, int ldy, const float* bias,
                              const float* bias1, int M, int N2, int K, void* stream) {
    return gemm_geglu_impl(true, A, lda, W, W1, H, ldh, Y, ldy, bias, bias1, M, N2, K, stream);
}
int sidlsg_gemm_geglu_bwd_bf16_g2(const void* dOut, int lda, const void* Wt, const void* Wt1, const void* H, void* dH, int ldh, int M, int F, int K,
                                  void* stream) {
    return gemm_geglu_bwd_impl(true, dOut, lda, Wt, Wt1, H, dH, ldh, M, F, K, stream);
}

// Implicit-GEMM 3x3 convolution, pad 1, NHWC.  X: [B][Hs][Ws][ldx] (ldx >= Cin, pixel stride),
// W: [Cout][3][3][Cin], Y: [B][Ho][Wo][ldc].  `ups`=1 reads X through a nearest x2 upsample
// (virtual input H x Wd = 2Hs x 2Ws).  stride in {1,2}.
static int conv3x3_bf16_impl(bool g2, const void* X, int ldx, const void* W, const void* W1, void* Y, int ldc, const float* bias, const float* bias1,
                             const void* res, int ldres, const float* rowvec, int ld_rowvec, int B, int H, int Wd, int Cin, int Cout, int stride,
                             int ups, float alpha, int flags, void* stream) {
    if ((stride != 1 && stride != 2) || (Cin & 7) || (ups && ((H | Wd) & 1))) return SIDLSG_EINVAL;
    if (g2 && !group2_args_ok(B, W1, bias, bias1)) return SIDLSG_EINVAL;
    GemmParams p = conv_params(X, ldx, W, Y, ldc, bias, res, ldres, rowvec, ld_rowvec, B, H, Wd, Cin, Cout, stride, ups, alpha, flags);
    if (int e = check_common(p)) return e;
    if (!range31(p.a_bytes, conv_src_pixels(B, H, Wd, ups), ldx, Cin, 2) || !range31(p.w_bytes, 9ull * Cout, Cin, Cin, 2)) return SIDLSG_EINVAL;
    set_group2(p, g2, W1, nullptr, bias1);
    if (int e = check_epilogue(p)) return e;
    if (Cin % 64 == 0) return dispatch_gemm<1>(p, (hipStream_t)stream);
    return dispatch_gemm<2>(p, (hipStream_t)stream);
}
int sidlsg_conv3x3_bf16(const void* X, int ldx, const void* W, void* Y, int ldc, const float* bias, const void* res,
                        int ldres, const float* rowvec, int ld_rowvec, int B, int H, int Wd, int Cin, int Cout, int stride,
                        int ups, float alpha, int flags, void* stream) {
    return conv3x3_bf16_impl(false, X, ldx, W, nullptr, Y, ldc, bias, nullptr, res, ldres, rowvec, ld_rowvec, B, H, Wd, Cin, Cout, stride, ups, alpha,
                             flags, stream);
}
// Grouped 3x3 convolution: samples [0, B/2) use (W, bias), samples [B/2, B) use (W1, bias1) (B even).
int sidlsg_conv3x3_bf16_g2(const void* X, int ldx, const void* W, const void* W1, void* Y, int ldc, const float* bias, const float* bias1,
                           const void* res, int ldres, const float* rowvec, int ld_rowvec, int B, int H, int Wd, int Cin, int Cout,
                           int stride, int ups, float alpha, int flags, void* stream) {
    return conv3x3_bf16_impl(true, X, ldx, W, W1, Y, ldc, bias, bias1, res, ldres, rowvec, ld_rowvec, B, H, Wd, Cin, Cout, stride, ups, alpha, flags,
                             stream);
}

// diffusers Downsample2D(padding = 0) of the AutoencoderKL encoder: F.pad(x, (0, 1, 0, 1)) then conv2d(k = 3, stride 2, no padding), i.e.
//   Y(i, j) = sum_{u, v} W(u, v) X(2 i + u, 2 j + v),   X = 0 at row H and column Wd          (H, Wd even; Y: [B][H/2][Wd/2][ldc])
// Forward only, bias epilogue (flags: SIDLSG_OUT_F32 | SIDLSG_SILU).  Its own entry point and its own kernel instantiations (PAD = 0 of
// gemm_bf16_kernel): the dispatch of sidlsg_conv3x3_bf16 is not involved.
int sidlsg_conv3x3_br_bf16(const void* X, int ldx, const void* W, void* Y, int ldc, const float* bias, int B, int H, int Wd, int Cin, int Cout,
                           int flags, void* stream) {
    if (B <= 0 || H <= 0 || Wd <= 0 || ((H | Wd) & 1) || (Cin & 7) || (flags & ~(F_OUT_F32 | F_SILU))) return SIDLSG_EINVAL;
    GemmParams p = conv_params(X, ldx, W, Y, ldc, bias, nullptr, 0, nullptr, 0, B, H, Wd, Cin, Cout, 2, 0, 1.0f, flags);      // Ho = H / 2, Wo = Wd / 2
    p.Mtot = p.M;
    if (int e = check_common(p)) return e;
    if (ldx < Cin || ldc < Cout) return SIDLSG_EINVAL;
    if (!range31(p.a_bytes, conv_src_pixels(B, H, Wd, 0), ldx, Cin, 2) || !range31(p.w_bytes, 9ull * Cout, Cin, Cin, 2)) return SIDLSG_EINVAL;
    SidlsgTraceScope ts(SIDLSG_FAM_CONV, 2.0 * p.M * (double)p.N * p.K,
                        2.0 * ((double)B * H * Wd * Cin + (double)p.N * p.K + (double)p.M * p.N * ((flags & F_OUT_F32) ? 2 : 1)));
    // 128 x 128 tiles once they cover the chip (>= 384: the rule of dispatch_gemm), 64 x 64 below
    const bool big = (long long)((p.M + 127) / 128) * ((p.N + 127) / 128) >= 384;
    hipStream_t s = (hipStream_t)stream;
    if (Cin % 64 == 0) return big ? launch_gemm<128, 128, 1, 0>(p, s) : launch_gemm<64, 64, 1, 0>(p, s);
    return big ? launch_gemm<128, 128, 2, 0>(p, s) : launch_gemm<64, 64, 2, 0>(p, s);
}

}  // extern "C"
