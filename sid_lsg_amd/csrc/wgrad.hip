// Weight (+ bias) gradients of the dense and conv3x3 contractions for gfx950 (MI355X): sidlsg_*wgrad*.
//   wgrad_v2_kernel / _v2w / _v2s / _v2f / _v2wf   direct-to-LDS staging, transpose reads (128 / 160-wide tiles, constant-advance conv gather)
//   wgrad_v2g_kernel / _v2sg                       several dense jobs in one launch
//   wgrad_bf16_kernel                              unaligned / ragged operands
//   wgrad_reduce_kernel / _reduce_g                fold the pixel-split slabs in one fixed order
// The loader conventions, DMA helpers and measurement switches are gemm_core.h's.
#include "gemm_core.h"

#ifdef SIDLSG_EXP_TRACE           // (measurement build) this unit's half of sidlsg_exp_set_trace
int sidlsg_exp_set_trace_wgrad(void* ptr) { return exp_set_trace_here(ptr); }
#endif

// ---------------------------------------------------------------------------------------------
// Weight gradient:  dW[N][K] += sum_m dY[m][N] * A[m][K]     (split over m; partial sums in fp32 slabs)
//
// Both operands are stored pixel-major, i.e. the contraction index m is the ROW of both LDS
// tiles.  MFMA wants 8 consecutive contraction elements per lane, so fragments are fetched
// with gfx950's LDS transpose read (ds_read_b64_tr_b16): a 16-lane group reads a
// [4 m][16 cols] block and lane i receives column i.  Two reads (m+0..3, m+4..7) give the
// 8-element fragment of the 16x16x32 MFMA for both operands, in the same m order.
// LDS rows are 256 B (128 columns); the 32-byte granule index is XOR-swizzled with
// (m&3)|((m>>3)&1)<<2 so the 8 rows a 32-lane half touches fall on 8 distinct granules.
constexpr int WG_T = 128;   // output tile: 128 (n) x 128 (k)
constexpr int WG_MB = 64;   // contraction rows per LDS stage

struct WgradParams {
    const bf16* dY;  // [M][ldy]
    const bf16* A;   // dense [M][lda] or NHWC image
    float* dW;       // [N][K]
    int M, N, K, ldy, lda;
    int H, Wd, Cin, Ho, Wo, stride, ups;
    int m_per_split;
    unsigned a_bytes, y_bytes;
    float* ws;        // [splits][N][K] slabs when splits > 1 and a workspace is available (else fp32 atomics)
    int nsplits;
    float* dB;        // optional: dB[n] += sum_m dY[m][n] (bias gradient), produced by the k-tile-0 blocks
    int slow_gather;  // conv: 1 = per-stage recomputation of the gather offsets also where the constant-advance path applies (A/B switch)
    int assign;       // dW = instead of dW +=: the caller knows dW holds nothing to keep (sidlsg_*wgrad_assign_bf16) -- no read of dW
    int bid0;         // grouped launch (wgrad_v2g_kernel): index of this job's first block (a multiple of 8); 0 otherwise
};

DEVFN int wg_swz(int row) { return (row & 3) | (((row >> 3) & 1) << 2); }

template <int MODE>
__global__ __launch_bounds__(NTHREADS) void wgrad_bf16_kernel(WgradParams p) {
    __shared__ __attribute__((aligned(16))) bf16 Ys[2][WG_MB][WG_T];
    __shared__ __attribute__((aligned(16))) bf16 Xs[2][WG_MB][WG_T];
    const int tiles_k = (p.K + WG_T - 1) / WG_T;
    const int tile = blockIdx.x;
    const int n0 = (tile / tiles_k) * WG_T, k0 = (tile % tiles_k) * WG_T;
    const int mbeg = blockIdx.y * p.m_per_split;
    const int mend = min(p.M, mbeg + p.m_per_split);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lg = lane >> 4;
    const int wn0 = (wave >> 1) * 64, wk0 = (wave & 1) * 64;
    const int c16 = tid & 15, r0 = tid >> 4;  // chunk column (8 elements) and first row

    const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16*>(p.A), 0, (int)p.a_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16*>(p.dY), 0, (int)p.y_bytes, 0x00020000);

    // per-thread constants of the A (k) operand: k is fixed for the whole kernel
    const int kA = k0 + c16 * 8;
    const bool kok = kA < p.K;
    int tap = 0, cA = kA, dh = 0, dw = 0;
    if (MODE == 1) { tap = kA / p.Cin; cA = kA - tap * p.Cin; dh = tap / 3; dw = tap - dh * 3; }
    const int nY = n0 + c16 * 8;
    const bool nfull = nY + 8 <= p.N;   // whole 16-byte chunk in range (else: ragged N, element path)
    const bool nany = nY < p.N;
    const int Hs = p.ups ? (p.H >> 1) : p.H, Ws = p.ups ? (p.Wd >> 1) : p.Wd;
    const int hw = (MODE == 1) ? p.Ho * p.Wo : 1;

    // conv: (b, ho, wo) of each of this thread's 4 rows, advanced by WG_MB pixels per step (no per-step divisions)
    int pb[4], pho[4], pwo[4];
    const int d_b = WG_MB / hw, d_rem = WG_MB - d_b * hw;
    const int d_ho = (MODE == 1) ? d_rem / p.Wo : 0, d_wo = (MODE == 1) ? d_rem - d_ho * p.Wo : 0;
    if (MODE == 1) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int m = mbeg + r0 + 16 * i;
            pb[i] = m / hw;
            const int rem = m - pb[i] * hw;
            pho[i] = rem / p.Wo;
            pwo[i] = rem - pho[i] * p.Wo;
        }
    }
    bf16x8 yreg[4], xreg[4];
    auto load_tile = [&](int mb) {      // called with mb = mbeg, mbeg + WG_MB, ... in order
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int m = mb + r0 + 16 * i;
            const bool mok = m < mend;
            if (nfull) {
                yreg[i] = buf_ld8(ry, mok ? ((unsigned)m * (unsigned)p.ldy + (unsigned)nY) * 2u : OOB);
            } else {
                bf16x8 v = zero8();
                if (nany && mok)
                    for (int e = 0; e < 8; e++) if (nY + e < p.N) v[e] = p.dY[(size_t)m * p.ldy + nY + e];
                yreg[i] = v;
            }
            if (MODE == 0) {
                xreg[i] = buf_ld8(ra, (kok && mok) ? ((unsigned)m * (unsigned)p.lda + (unsigned)kA) * 2u : OOB);
            } else {
                bool ok = kok && mok;
                const int b = pb[i], ho = pho[i], wo = pwo[i];
                int hi = ho * p.stride - 1 + dh, wi = wo * p.stride - 1 + dw;
                ok = ok && hi >= 0 && hi < p.H && wi >= 0 && wi < p.Wd;
                if (p.ups) { hi >>= 1; wi >>= 1; }
                xreg[i] = buf_ld8(ra, ok ? (((unsigned)(b * Hs + hi) * (unsigned)Ws + (unsigned)wi) * (unsigned)p.lda + (unsigned)cA) * 2u : OOB);
                // advance this row by WG_MB pixels: (b, ho, wo) += (d_b, d_ho, d_wo) with single carries
                int nwo = wo + d_wo, nho = ho + d_ho, nb = b + d_b;
                if (nwo >= p.Wo) { nwo -= p.Wo; nho += 1; }
                if (nho >= p.Ho) { nho -= p.Ho; nb += 1; }
                pwo[i] = nwo; pho[i] = nho; pb[i] = nb;
            }
        }
    };
    auto store_tile = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int r = r0 + 16 * i;
            const int col = ((((c16 >> 1) ^ wg_swz(r)) << 1) | (c16 & 1)) << 3;
            st8(&Ys[buf][r][col], yreg[i]);
            st8(&Xs[buf][r][col], xreg[i]);
        }
    };

    f32x4 acc[4][4];   // [n tile][k tile]
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // bias gradient = dY^T * ones: one extra MFMA per dY fragment in the waves that own k-columns 0..63 of k-tile 0
    const bool do_bias = p.dB != nullptr && k0 == 0 && wk0 == 0;
    f32x4 accb[4];
#pragma unroll
    for (int i = 0; i < 4; i++) accb[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const bf16x8 ones = {f2bf(1.f), f2bf(1.f), f2bf(1.f), f2bf(1.f), f2bf(1.f), f2bf(1.f), f2bf(1.f), f2bf(1.f)};

    typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
    auto tr_frag = [&](const bf16* tilebase, int mrow, int colbase) -> bf16x8 {
        // lane t=(li) of group lg addresses row mrow + 8*lg + (t>>2) (+4 for the 2nd read), 4 columns at (t&3)*4
        const int rA = mrow + 8 * lg + (li >> 2);
        const int rB = rA + 4;
        const int g = colbase >> 4;                  // 16-column granule of this fragment
        const int ca = ((g ^ wg_swz(rA)) << 4) + (li & 3) * 4;
        const int cb = ((g ^ wg_swz(rB)) << 4) + (li & 3) * 4;
        s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(tilebase + rA * WG_T + ca));
        s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(tilebase + rB * WG_T + cb));
        typedef short s16x8 __attribute__((ext_vector_type(8)));
        s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        return __builtin_bit_cast(bf16x8, v);
    };

    const int nsteps = (mend - mbeg + WG_MB - 1) / WG_MB;
    if (nsteps <= 0) return;
    load_tile(mbeg);
    store_tile(0);
    __syncthreads();
    for (int st = 0; st < nsteps; st++) {
        const int buf = st & 1;
        if (st + 1 < nsteps) load_tile(mbeg + (st + 1) * WG_MB);
#pragma unroll
        for (int kk = 0; kk < 2; kk++) {
            bf16x8 fy[4], fx[4];
#pragma unroll
            for (int i = 0; i < 4; i++) fy[i] = tr_frag(&Ys[buf][0][0], kk * 32, wn0 + i * 16);
#pragma unroll
            for (int j = 0; j < 4; j++) fx[j] = tr_frag(&Xs[buf][0][0], kk * 32, wk0 + j * 16);
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 4; j++)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fy[i], fx[j], acc[i][j], 0, 0, 0);
            if (do_bias) {
#pragma unroll
                for (int i = 0; i < 4; i++) accb[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fy[i], ones, accb[i], 0, 0, 0);
            }
        }
        if (st + 1 < nsteps) store_tile(buf ^ 1);
        __syncthreads();
    }
    if (do_bias && li == 0) {
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int n = n0 + wn0 + 16 * i + lg * 4 + r;
                if (n < p.N) unsafeAtomicAdd(p.dB + n, accb[i][r]);
            }
    }
    // acc[i][j][r]: n = n0+wn0+16i + lg*4 + r ; k = k0+wk0+16j + li
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int k = k0 + wk0 + 16 * j + li;
            if (k >= p.K) continue;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int n = n0 + wn0 + 16 * i + lg * 4 + r;
                if (n >= p.N) continue;
                const size_t e = (size_t)n * p.K + k;
                if (p.nsplits == 1) p.dW[e] = p.assign ? acc[i][j][r] : p.dW[e] + acc[i][j][r];   // sole owner of this element
                else if (p.ws) p.ws[(size_t)blockIdx.y * p.N * p.K + e] = acc[i][j][r];      // slab, reduced by wgrad_reduce_kernel
                else unsafeAtomicAdd(p.dW + e, acc[i][j][r]);
            }
        }
}


// "wgrad v2": same tile, LDS layout and fragment reads as wgrad_bf16_kernel, but the dY / X tiles are staged by
// direct-to-LDS loads (global_load_lds_dwordx4): no staging registers, no ds_write commit phase.  The LDS swizzle is
// applied on the SOURCE side: lane (row, q) fetches the 16-byte chunk whose swizzled position is q.  Padding (rows past
// the split, columns past N/K, conv halo) reads a zero page.  Schedule per 64-pixel stage (2 LDS buffers, one barrier):
//   A: issue the kk=1 fragment reads of the current buffer; kk=0 MFMAs   C: vmcnt(0)+lgkmcnt(0); s_barrier
//   D: kk=0 fragment reads of the next buffer; DMA of stage st+2 into the buffer just vacated   E: kk=1 MFMAs
// Blocks are numbered split-major and remapped so that one XCD works on consecutive (split, tile) pairs: the tiles of a
// split share the same dY / X rows (the 9 taps re-read X shifted), which then stay in that XCD's L2.
// Requires N % 8 == 0, K % 8 == 0 (conv: Cin % 8 == 0), ldy % 8 == 0, lda % 8 == 0, 16-byte aligned bases.
// TN = n (dY column) extent of the tile: 160 when N % 160 == 0 (every SD channel count: 320 = 2 tiles instead of 3 of 128),
// else 128.  The k (X column) extent stays 128.
template <int TN> DEVFN int wg_yswz(int row) { return TN == 128 ? wg_swz(row) : ((row >> 3) & 1); }

// TK = k (X column) extent of the tile: 128, or (dense only, round 4) 160 -- with N and K multiples of 160 a 160 x 160 tile wastes no
// MFMA work on padding (320 = 2 x 160 instead of 3 x 128) and the operands are re-read 2 + 2 instead of 3 + 3 times per split
// (L2 -> LDS bytes -44 % at 320 x 320); the X tile is then staged exactly like the dY tile (same chunk grid, same swizzle).
// (TAG: hipcc 7.2's host pass rejects the SECOND kernel that instantiates one specialisation of this template -- "no matching function,
// substitution failure", as it did for attn_q_kernel -- so the grouped kernel asks for its own, TAG = 1)
template <int MODE, int TN, int TK, bool CF = false, int TAG = 0>      // CF: conv with constant-advance gather offsets (see fastc below; the host checks the conditions)
DEVFN void wgrad_v2_body(const WgradParams& p) {
    static_assert(TK == WG_T || (TK == 160 && MODE == 0), "160-wide k tiles: dense operands only");
    constexpr int KI = TK / 32;             // 16-column X fragments per wave (wave = TN/2 x TK/2 of the tile)
    constexpr int XC = TK / 8;              // 16-byte chunks per X row (TK = 160 staging)
    constexpr int NI = TN / 32;             // 16-column dY fragments per wave (wave = TN/2 x 64 of the tile)
    constexpr int YI = TN / 32;             // dY DMA instructions per wave and stage (64 rows x TN/8 chunks / 256 lanes)
    constexpr int YC = TN / 8;              // 16-byte chunks per dY row
    constexpr int STAGE = WG_MB * (TN + TK);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    bf16* ring = reinterpret_cast<bf16*>(smem);
    const int tiles_k = (p.K + TK - 1) / TK;
    const int tiles = ((p.N + TN - 1) / TN) * tiles_k;
    const int bid = xcd_contiguous((int)blockIdx.x - p.bid0, tiles * p.nsplits);      // (bid0: first block of this job in a grouped launch, else 0)
    const int split = bid / tiles, tile = bid - split * tiles;
    const int n0 = (tile / tiles_k) * TN, k0 = (tile % tiles_k) * TK;
    const int mbeg = split * p.m_per_split;
    const int mend = min(p.M, mbeg + p.m_per_split);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, lg = lane >> 4;
    const int wn0 = (wave >> 1) * (TN / 2), wk0 = (wave & 1) * (TK / 2);
    const int q16 = tid & 15, r0 = tid >> 4;            // LDS chunk position and first row of this lane
    const int c16 = (((q16 >> 1) ^ wg_swz(r0)) << 1) | (q16 & 1);   // source chunk (wg_swz(r0 + 16 i) == wg_swz(r0))
    const int kA = k0 + c16 * 8;
    const bool kok = kA < p.K;
    int cA = kA, dh = 0, dw = 0;
    if (MODE == 1) { const int tap = kA / p.Cin; cA = kA - tap * p.Cin; dh = tap / 3; dw = tap - dh * 3; }
    const int Hs = p.ups ? (p.H >> 1) : p.H, Ws = p.ups ? (p.Wd >> 1) : p.Wd;
    const int hw = (MODE == 1) ? p.Ho * p.Wo : 1;
    // buffer_load ... lds with one 32-bit byte offset per row; rows past the split / columns past N,K / the conv halo
    // carry an out-of-range offset (the buffer unit writes zeros).  dY and dense X advance by a wave-uniform soffset.
    const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16*>(p.dY), 0, (int)p.y_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16*>(p.A), 0, (int)p.a_bytes, 0x00020000);
    // dY: DMA instruction j of wave w fills LDS chunks [(w*YI + j)*64, +64) of the [64][YC] chunk grid; the lane's
    // position (row, cpos) holds the source chunk whose swizzled position it is
    unsigned yoff[YI], xoff[4];
#pragma unroll
    for (int j = 0; j < YI; j++) {
        const int idx = (wave * YI + j) * 64 + lane;
        const int row = idx / YC, cpos = idx - row * YC;
        const int chunk = (((cpos >> 1) ^ wg_yswz<TN>(row)) << 1) | (cpos & 1);
        const int nY = n0 + chunk * 8;
        yoff[j] = nY < p.N ? ((unsigned)(mbeg + row) * (unsigned)p.ldy + (unsigned)nY) * 2u : OOB;
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const unsigned m = (unsigned)(mbeg + r0 + 16 * i);
        xoff[i] = (MODE == 0 && kok) ? (m * (unsigned)p.lda + (unsigned)kA) * 2u : OOB;
    }
    unsigned xoffw[TK == WG_T ? 1 : KI];         // TK = 160: the dY scheme for X (KI DMA instructions per wave and stage)
    if constexpr (TK != WG_T) {
#pragma unroll
        for (int j = 0; j < KI; j++) {
            const int idx = (wave * KI + j) * 64 + lane;
            const int row = idx / XC, cpos = idx - row * XC;
            const int chunk = (((cpos >> 1) ^ wg_yswz<TK>(row)) << 1) | (cpos & 1);
            const int kX = k0 + chunk * 8;
            xoffw[j] = kX < p.K ? ((unsigned)(mbeg + row) * (unsigned)p.lda + (unsigned)kX) * 2u : OOB;
        }
    }

    int pb[4], pho[4], pwo[4];
    const int d_b = WG_MB / hw, d_rem = WG_MB - d_b * hw;
    const int d_ho = (MODE == 1) ? d_rem / p.Wo : 0, d_wo = (MODE == 1) ? d_rem - d_ho * p.Wo : 0;
    if (MODE == 1) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int m = mbeg + r0 + 16 * i;
            pb[i] = m / hw;
            const int rem = m - pb[i] * hw;
            pho[i] = rem / p.Wo;
            pwo[i] = rem - pho[i] * p.Wo;
        }
    }
    // conv fast path (round 4): when a stage's 64 pixels are whole image rows or whole samples (Wo | 64 or Ho * Wo | 64: every SD shape),
    // the stride divides the image (H == Ho * stride) and there is no fused upsampling, the input row of a lane's pixel advances by the
    // SAME number of rows every stage -- also across sample boundaries -- so the gather offset is a per-lane constant plus a wave-uniform
    // soffset (as in the dense kernel) and only the vertical halo test remains per stage: ~9 instead of ~40 VALU per row and stage
    // (the conv weight gradient ran 5.3 VALU instructions per MFMA, profiles/r04_wgrad_sq_pmc.json).  The descriptor's base sits one
    // image row below X so that the offset of a pixel in the top halo row is not negative.
    const unsigned rowb = (unsigned)Ws * (unsigned)p.lda * 2u;
    constexpr bool fastc = CF;      // (as a run-time branch beside the general path the kernel lost 35 %: two gather bodies in the stage loop)
    static_assert(!CF || (MODE == 1 && TK == WG_T), "constant-advance gather: conv, 128-column k tiles");
    const __amdgpu_buffer_rsrc_t rxf = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16*>(p.A) - (fastc ? (size_t)rowb / 2 : 0), 0,
                                                                         (int)(p.a_bytes + (fastc ? rowb : 0u)), 0x00020000);
    const int dstage = fastc ? (d_b * p.H + d_ho * p.stride) * (int)rowb : 0;
    unsigned xoffc[4];
    if constexpr (fastc) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int wi = pwo[i] * p.stride - 1 + dw;
            const bool wok = kok && wi >= 0 && wi < p.Wd;
            xoffc[i] = wok ? ((unsigned)(pb[i] * p.H + pho[i] * p.stride + dh) * rowb + ((unsigned)wi * (unsigned)p.lda + (unsigned)cA) * 2u) : OOB;
        }
    }
    auto issue = [&](int mb, int buf) {      // called with mb = mbeg, mbeg + WG_MB, ... in order; YI + 4 DMA instructions per wave
        bf16* ys = ring + buf * STAGE;
        bf16* xs = ys + WG_MB * TN;
        const int ysoff = (mb - mbeg) * p.ldy * 2, xsoff = (mb - mbeg) * p.lda * 2;
        const bool tail = mb + WG_MB > mend;          // only the last stage of a split has rows past mend
#pragma unroll
        for (int j = 0; j < YI; j++) {
            const bool mok = !tail || (mb + ((wave * YI + j) * 64 + lane) / YC < mend);
            if (SIDLSG_WGRAD_ASM_DMA) dma16_asm(ry, ys + (wave * YI + j) * 512, mok ? yoff[j] : OOB, ysoff);
            else __builtin_amdgcn_raw_ptr_buffer_load_lds(ry, (lptr_t)(ys + (wave * YI + j) * 512), 16, mok ? yoff[j] : OOB, ysoff, 0, 0);
        }
        if constexpr (TK != WG_T) {
#pragma unroll
            for (int j = 0; j < KI; j++) {
                const bool mok = !tail || (mb + ((wave * KI + j) * 64 + lane) / XC < mend);
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (lptr_t)(xs + (wave * KI + j) * 512), 16, mok ? xoffw[j] : OOB, xsoff, 0, 0);
            }
            return;
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const bool mok = !tail || (mb + r0 + 16 * i < mend);
            if (MODE == 0) {
                if (SIDLSG_WGRAD_ASM_DMA) dma16_asm(rx, xs + (4 * wave + 16 * i) * WG_T, mok ? xoff[i] : OOB, xsoff);
                else __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (lptr_t)(xs + (4 * wave + 16 * i) * WG_T), 16, mok ? xoff[i] : OOB, xsoff, 0, 0);
            } else if constexpr (fastc) {
                const int ho = pho[i];
                const int hi = ho * p.stride - 1 + dh;
                const bool ok = mok && hi >= 0 && hi < p.H;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rxf, (lptr_t)(xs + (4 * wave + 16 * i) * WG_T), 16, ok ? xoffc[i] : OOB,
                                                         ((mb - mbeg) / WG_MB) * dstage, 0, 0);
                const int nho = ho + d_ho;
                pho[i] = nho >= p.Ho ? nho - p.Ho : nho;
            } else {
                bool ok = kok && mok;
                const int b = pb[i], ho = pho[i], wo = pwo[i];
                int hi = ho * p.stride - 1 + dh, wi = wo * p.stride - 1 + dw;
                ok = ok && hi >= 0 && hi < p.H && wi >= 0 && wi < p.Wd;
                if (p.ups) { hi >>= 1; wi >>= 1; }
                const unsigned o = ok ? (((unsigned)(b * Hs + hi) * (unsigned)Ws + (unsigned)wi) * (unsigned)p.lda + (unsigned)cA) * 2u : OOB;
                if (SIDLSG_WGRAD_ASM_DMA) dma16_asm(rx, xs + (4 * wave + 16 * i) * WG_T, o, 0);
                else __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (lptr_t)(xs + (4 * wave + 16 * i) * WG_T), 16, o, 0, 0, 0);
                int nwo = wo + d_wo, nho = ho + d_ho, nb = b + d_b;
                if (nwo >= p.Wo) { nwo -= p.Wo; nho += 1; }
                if (nho >= p.Ho) { nho -= p.Ho; nb += 1; }
                pwo[i] = nwo; pho[i] = nho; pb[i] = nb;
            }
        }
    };

    f32x4 acc[NI][KI];   // [n tile][k tile]
#pragma unroll
    for (int i = 0; i < NI; i++)
#pragma unroll
        for (int j = 0; j < KI; j++) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const bool do_bias = p.dB != nullptr && k0 == 0 && wk0 == 0;
    f32x4 accb[NI];
#pragma unroll
    for (int i = 0; i < NI; i++) accb[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const bf16x8 ones = {f2bf(1.f), f2bf(1.f), f2bf(1.f), f2bf(1.f), f2bf(1.f), f2bf(1.f), f2bf(1.f), f2bf(1.f)};

    typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
    // per-lane LDS offsets of the two transpose reads of a fragment (rows 8*lg + (li>>2) and +4), excluding the
    // 16-column granule g of the fragment, which enters as (g ^ swz) << 4
    const int rA = 8 * lg + (li >> 2), rB = rA + 4;
    // kk*32 does not change the swizzle bits.  X tile: 256-byte rows, 3-bit granule XOR; dY tile: TN*2-byte rows (320 B
    // rows alias the banks of rows 8 apart only -> 1-bit XOR with (row>>3)&1 for TN = 160)
    const int sxA = wg_yswz<TK>(rA), sxB = wg_yswz<TK>(rB), syA = wg_yswz<TN>(rA), syB = wg_yswz<TN>(rB);
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    auto tr_frag = [&](const bf16* tilebase, int pitch, int sA, int sB, int kk, int colbase) -> bf16x8 {
        const int g = colbase >> 4;
        const bf16* base = tilebase + kk * 32 * pitch + (li & 3) * 4;
        s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(base + rA * pitch + ((g ^ sA) << 4)));
        s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(base + rB * pitch + ((g ^ sB) << 4)));
        s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        return __builtin_bit_cast(bf16x8, v);
    };
    auto read_frags = [&](int buf, int kk, bf16x8 (&fy)[NI], bf16x8 (&fx)[KI]) {
        const bf16* ys = ring + buf * STAGE;
        const bf16* xs = ys + WG_MB * TN;
#pragma unroll
        for (int i = 0; i < NI; i++) fy[i] = tr_frag(ys, TN, syA, syB, kk, wn0 + i * 16);
#pragma unroll
        for (int j = 0; j < KI; j++) fx[j] = tr_frag(xs, TK, sxA, sxB, kk, wk0 + j * 16);
    };
    auto mfma_block = [&](const bf16x8 (&fy)[NI], const bf16x8 (&fx)[KI]) {
        if constexpr ((SIDLSG_V3_PRIO) & 2) V3_SETPRIO(1);
#pragma unroll
        for (int i = 0; i < NI; i++)
#pragma unroll
            for (int j = 0; j < KI; j++)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fy[i], fx[j], acc[i][j], 0, 0, 0);
        if (do_bias) {
#pragma unroll
            for (int i = 0; i < NI; i++) accb[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fy[i], ones, accb[i], 0, 0, 0);
        }
        if constexpr ((SIDLSG_V3_PRIO) & 2) V3_SETPRIO(0);
    };

    const int nsteps = (mend - mbeg + WG_MB - 1) / WG_MB;
    if (nsteps <= 0) return;
    bf16x8 fy0[NI], fx0[KI], fy1[NI], fx1[KI];
    WTRACE(0);
    issue(mbeg, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    WTRACE(1);
    read_frags(0, 0, fy0, fx0);
    if (nsteps > 1) issue(mbeg + WG_MB, 1);
    auto stage = [&](const int st, auto has_next, auto fetch) {           // straight-line instantiations: see gemm_v3_kernel
        const int buf = st & 1;
        read_frags(buf, 1, fy1, fx1);                                     // A
        mfma_block(fy0, fx0);
        if (SIDLSG_V3_SCHED_FENCE) __builtin_amdgcn_sched_barrier(0);    // keep the kk=0 MFMAs in front of the wait
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");      // C: my DMA share of stage st+1 landed; my reads of buf done
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (SIDLSG_V3_SCHED_FENCE) __builtin_amdgcn_sched_barrier(0);
        if constexpr (decltype(has_next)::value) {                        // D
            read_frags(buf ^ 1, 0, fy0, fx0);
            if constexpr (decltype(fetch)::value) issue(mbeg + (st + 2) * WG_MB, buf);
        }
        mfma_block(fy1, fx1);                                             // E
    };
    {
        int st = 0;
        for (; st + 2 < nsteps; st++) stage(st, std::true_type{}, std::true_type{});
        if (st + 1 < nsteps) { stage(st, std::true_type{}, std::false_type{}); st++; }
        stage(st, std::false_type{}, std::false_type{});
    }
    WTRACE(2);
    if (do_bias && li == 0) {
#pragma unroll
        for (int i = 0; i < NI; i++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int n = n0 + wn0 + 16 * i + lg * 4 + r;
                if (n < p.N) unsafeAtomicAdd(p.dB + n, accb[i][r]);
            }
    }
    // Result write-out.  In the accumulator layout a lane holds single floats of 16-float row segments: 64-80 scalar stores
    // per lane behind three run-time branches each -- the phase trace (tools/ab/wgrad_trace.py) showed 7.5-18 us per block in
    // this epilogue, a third to a half of a dense weight-gradient block.  Instead the tile goes through LDS (the stage ring is
    // free now; fp32 [TN/2][128 + 4], one half of the n rows at a time) and leaves as 16-byte stores along k: 512-byte runs
    // (11.5 -> 9.3 us dense, 9.6 -> 5.9 us conv; code 19.8 -> 11.2 KB).  What remains is a chip-wide write burst: all blocks of
    // a launch have equal work, reach this point together and write tiles x splits x 64 KB of slabs (31 MB for 65536x320x320)
    // with nothing left to overlap it.
    if (p.nsplits == 1 || p.ws) {
        constexpr int LDW = TK + 4;
        float* img = reinterpret_cast<float*>(smem);
        float* dst = p.nsplits == 1 ? p.dW : p.ws + (size_t)split * p.N * p.K;
        const bool accum = p.nsplits == 1 && !p.assign;
#pragma unroll
        for (int h = 0; h < 2; h++) {
            __syncthreads();                             // the ring (or the previous half image) is no longer read
            if ((wave >> 1) == h) {
#pragma unroll
                for (int i = 0; i < NI; i++)
#pragma unroll
                    for (int j = 0; j < KI; j++)
#pragma unroll
                        for (int r = 0; r < 4; r++) img[(16 * i + lg * 4 + r) * LDW + wk0 + 16 * j + li] = acc[i][j][r];
            }
            __syncthreads();
            for (int c = tid; c < (TN / 2) * (TK / 4); c += NTHREADS) {
                const int row = c / (TK / 4), k4 = (c - row * (TK / 4)) * 4;
                const int n = n0 + h * (TN / 2) + row, k = k0 + k4;
                if (n < p.N && k < p.K) {
                    f32x4 v = *reinterpret_cast<const f32x4*>(img + row * LDW + k4);
                    float* d = dst + (size_t)n * p.K + k;
                    if (accum) v += *reinterpret_cast<const f32x4*>(d);
                    *reinterpret_cast<f32x4*>(d) = v;
                }
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < NI; i++)
#pragma unroll
            for (int j = 0; j < KI; j++) {
                const int k = k0 + wk0 + 16 * j + li;
                if (k >= p.K) continue;
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int n = n0 + wn0 + 16 * i + lg * 4 + r;
                    if (n < p.N) unsafeAtomicAdd(p.dW + (size_t)n * p.K + k, acc[i][j][r]);
                }
            }
    }
    WTRACE(3);
#ifdef SIDLSG_EXP_TRACE
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    WTRACE(4);
#endif
}

// (two plain kernels over one body: a kernel template with the second non-type parameter did not get a host stub from
// hipcc 7.2 -- undefined symbol at load time, no diagnostic)
template <int MODE>
__global__ __launch_bounds__(NTHREADS, 2) void wgrad_v2_kernel(WgradParams p) { wgrad_v2_body<MODE, 128, WG_T>(p); }
template <int MODE>
__global__ __launch_bounds__(NTHREADS, 2) void wgrad_v2w_kernel(WgradParams p) { wgrad_v2_body<MODE, 160, WG_T>(p); }
__global__ __launch_bounds__(NTHREADS, 2) void wgrad_v2s_kernel(WgradParams p) { wgrad_v2_body<0, 160, 160>(p); }      // dense, 160 x 160 tiles
__global__ __launch_bounds__(NTHREADS, 2) void wgrad_v2f_kernel(WgradParams p) { wgrad_v2_body<1, 128, WG_T, true>(p); }     // conv, constant-advance gather
__global__ __launch_bounds__(NTHREADS, 2) void wgrad_v2wf_kernel(WgradParams p) { wgrad_v2_body<1, 160, WG_T, true>(p); }    // the same with 160-wide n tiles

// ---- grouped dense weight gradients (round 5) --------------------------------------------------------------------------------------
// The square projections of a transformer block (to_out of both attentions, the cross-attention's to_q, proj_in / proj_out: C x C, plus the
// 77-token k|v projection) each need ~56 pixel splits to fill the chip on their own (9 tiles of 128 x 128 at C = 320): per layer 31 MB of
// slabs, a reduce launch, and 49 + 16 us for 13 GFLOP.  wgrad_v2g_kernel runs up to WG_GROUP such layers in ONE grid -- every job keeps its
// own operands, shapes and split count (WgradParams by value in the kernel argument), a block finds its job from its index -- so that the
// group as a whole fills the chip with ~1/5 of the splits per layer, and wgrad_reduce_g_kernel folds all its slabs in one launch.
constexpr int WG_GROUP = 8;
struct WgradGroup { int njobs; int blk0[WG_GROUP + 1]; WgradParams j[WG_GROUP]; };      // blk0: first block of each job (multiples of 8)
__global__ __launch_bounds__(NTHREADS, 2) void wgrad_v2g_kernel(WgradGroup g) {
    const int bx = blockIdx.x;
    int j = 0;
#pragma unroll
    for (int i = 1; i < WG_GROUP; i++)
        if (i < g.njobs && bx >= g.blk0[i]) j = i;
    const WgradParams& p = g.j[j];          // (p.bid0 == g.blk0[j], set by the host)
    const int local = bx - g.blk0[j];
    const int nblk = (((p.N + 127) / 128) * ((p.K + WG_T - 1) / WG_T)) * p.nsplits;
    if (local >= nblk) return;              // (the job's range is padded to a multiple of 8 blocks: XCD = block index mod 8 inside a job too)
    wgrad_v2_body<0, 128, WG_T, false, 1>(p);
}
// the same for the layers of the 160 x 160-tile kernel (q|k|v, FF-in, FF-out: N and K multiples of 160)
__global__ __launch_bounds__(NTHREADS, 2) void wgrad_v2sg_kernel(WgradGroup g) {
    const int bx = blockIdx.x;
    int j = 0;
#pragma unroll
    for (int i = 1; i < WG_GROUP; i++)
        if (i < g.njobs && bx >= g.blk0[i]) j = i;
    const WgradParams& p = g.j[j];
    const int local = bx - g.blk0[j];
    const int nblk = ((p.N / 160) * (p.K / 160)) * p.nsplits;
    if (local >= nblk) return;
    wgrad_v2_body<0, 160, 160, false, 1>(p);
}
struct WgradReduceGroup { int njobs; unsigned blk0[WG_GROUP + 1]; const float* ws[WG_GROUP]; float* dW[WG_GROUP]; unsigned n4[WG_GROUP]; int splits[WG_GROUP], assign[WG_GROUP]; };
__global__ __launch_bounds__(256) void wgrad_reduce_g_kernel(WgradReduceGroup g) {
    int j = 0;
#pragma unroll
    for (int i = 1; i < WG_GROUP; i++)
        if (i < g.njobs && blockIdx.x >= g.blk0[i]) j = i;
    const unsigned i4 = (blockIdx.x - g.blk0[j]) * 256 + threadIdx.x;
    if (i4 >= g.n4[j]) return;
    const size_t i = (size_t)i4 * 4, n = (size_t)g.n4[j] * 4;
    const float* ws = g.ws[j];
    float* dW = g.dW[j];
    const int splits = g.splits[j];
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (!g.assign[j]) v = *reinterpret_cast<const f32x4*>(dW + i);
    int sidx = 0;
    for (; sidx + 3 < splits; sidx += 4) {          // wgrad_reduce_kernel's order: bit-identical sums
        const f32x4 a = *reinterpret_cast<const f32x4*>(ws + (size_t)sidx * n + i);
        const f32x4 b = *reinterpret_cast<const f32x4*>(ws + (size_t)(sidx + 1) * n + i);
        const f32x4 c = *reinterpret_cast<const f32x4*>(ws + (size_t)(sidx + 2) * n + i);
        const f32x4 d = *reinterpret_cast<const f32x4*>(ws + (size_t)(sidx + 3) * n + i);
        v += a; v += b; v += c; v += d;
    }
    for (; sidx < splits; sidx++) v += *reinterpret_cast<const f32x4*>(ws + (size_t)sidx * n + i);
    *reinterpret_cast<f32x4*>(dW + i) = v;
}

// dW[i] += sum_s slab[s][i]  (assign: dW[i] = sum_s slab[s][i], summed in the same order from 0 -- bit-identical to the sum onto a zeroed dW)
__global__ void wgrad_reduce_kernel(const float* __restrict__ ws, float* __restrict__ dW, size_t n, int splits, int assign) {
    const size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i + 4 <= n) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (!assign) v = *reinterpret_cast<const f32x4*>(dW + i);
        int sidx = 0;
        for (; sidx + 3 < splits; sidx += 4) {          // four independent slab loads in flight, fixed summation order
            const f32x4 a = *reinterpret_cast<const f32x4*>(ws + (size_t)sidx * n + i);
            const f32x4 b = *reinterpret_cast<const f32x4*>(ws + (size_t)(sidx + 1) * n + i);
            const f32x4 c = *reinterpret_cast<const f32x4*>(ws + (size_t)(sidx + 2) * n + i);
            const f32x4 d = *reinterpret_cast<const f32x4*>(ws + (size_t)(sidx + 3) * n + i);
            v += a; v += b; v += c; v += d;
        }
        for (; sidx < splits; sidx++) v += *reinterpret_cast<const f32x4*>(ws + (size_t)sidx * n + i);
        *reinterpret_cast<f32x4*>(dW + i) = v;
    } else {
        for (size_t j = i; j < n; j++) {
            float v = assign ? 0.f : dW[j];
            for (int sidx = 0; sidx < splits; sidx++) v += ws[(size_t)sidx * n + j];
            dW[j] = v;
        }
    }
}

// Dynamic LDS of the wgrad_v2* kernels: two stages of WG_MB contraction rows of a tn-wide dY tile and a tk-wide A tile
constexpr int wgrad_v2_lds(int tn, int tk) { return 2 * WG_MB * (tn + tk) * (int)sizeof(bf16); }

// A pixel split: M contraction rows over `splits` blocks -> rows per split in whole LDS stages (WG_MB rows) and the number of splits
// that many rows per split need (<= `splits`)
struct PixelSplit { int mps, splits; };
static PixelSplit pixel_split(int M, int splits) {
    const int mps = ((M + splits - 1) / splits + WG_MB - 1) / WG_MB * WG_MB;
    return {mps, (M + mps - 1) / mps};
}

// Deterministic mode, weight gradients: the pixel splits never meet in fp32 atomics.  dW: slabs + wgrad_reduce_kernel (split order) or
// one split when no two slabs fit; the bias: the k-tile-0 blocks of every split added into dB, so with several splits the kernel
// gets no dB and the bias gradient is an order-fixed column sum of dY (sidlsg_colsum, B = 1) after it.
template <int MODE>
static int launch_wgrad(WgradParams p, hipStream_t s) {
    static const bool v2_on = sidlsg_env_on("SIDLSG_WGRAD_V2");
    static const bool tn160_on = sidlsg_env_on("SIDLSG_WGRAD_TN160");   // A/B switch
    const bool aligned = !(p.N & 7) && !(p.K & 7) && !(p.ldy & 7) && !(p.lda & 7) && !(MODE == 1 && (p.Cin & 7)) &&
                         !(((uintptr_t)p.dY | (uintptr_t)p.A) & 15);
    const bool v2 = v2_on && aligned;
    // 160-wide n tiles: measured faster only where they cut the tile count by a third (conv, Cout = 320: 216 -> 178 us);
    // for N = 640 (5 -> 4 tiles) and the dense shapes the leaner 128 kernel wins
    static const bool tn160_dense = sidlsg_env_int("SIDLSG_WGRAD_TN160_DENSE", 0) != 0;   // A/B switch
    // dense, N and K multiples of 160 (every Linear of the SD transformer blocks): 160 x 160 tiles (wgrad_v2s_kernel)
    static const bool sq160_on = sidlsg_env_on("SIDLSG_WGRAD_SQ160");       // A/B switch
    // measured per shape (tools/ab/wgrad_sweep.py, MI355X): faster on every non-square layer of the transformer blocks at M >= 4096
    // (2560 x 320: 192 -> 157 us, 5120 x 640: 145 -> 120, 10240 x 1280: 139 -> 112; a backward pass's dense weight gradients 1025 -> 927 us
    // at CFG batch 16), slower on the square C x C layers (fewer, larger tiles need more pixel splits = more slab traffic: 36.7 -> 39.9 us)
    // and at small pixel counts unless the weight is very large
    const bool sq160 = v2 && sq160_on && MODE == 0 && p.N % 160 == 0 && p.K % 160 == 0 && p.N != p.K &&
                       (p.M >= 4096 || (long long)p.N * p.K >= (8ll << 20));
    const int tn = sq160 ? 160 : (v2 && tn160_on && (MODE == 1 || tn160_dense) && p.N == 320) ? 160 : WG_T;
    const int tk = sq160 ? 160 : WG_T;
    const int tiles = ((p.N + tn - 1) / tn) * ((p.K + tk - 1) / tk);
    // Split the pixel contraction so the grid fills the chip in whole rounds of 512 resident blocks (256 CUs x 2).
    // Small cost model (us): rounds * (rows per block * 24 ns + 3 us block overhead) + slab reduction at ~4 TB/s;
    // e.g. 69 tiles: ceil(768/69) = 12 splits ran 1.6 rounds, the model picks a whole number of rounds.
    int want = 1;
    {
        const int cap = std::min(64, (p.M + 4 * WG_MB - 1) / (4 * WG_MB));
        static const int slots = sidlsg_env_int("SIDLSG_WGRAD_SLOTS", 512);   // A/B knob: resident blocks a launch may count on
        double best = 1e30;
        const double slab_us = (double)p.N * p.K * 4.0 / 4e6;
        for (int sp = 1; sp <= cap; sp++) {
            const int rounds = (sp * tiles + slots - 1) / slots;
            const double rows = (double)((p.M + sp - 1) / sp);
            const double est = rounds * (rows * 0.024 + 3.0) + (sp > 1 ? sp * slab_us : 0.0);
            if (est < best) { best = est; want = sp; }
        }
    }
    const int max_splits = (p.M + 4 * WG_MB - 1) / (4 * WG_MB);
    if (want > max_splits) want = max_splits;
    if (want < 1) want = 1;
    PixelSplit ps = pixel_split(p.M, want);
    const long long nk = (long long)p.N * p.K;
    const Ws wsl = ws_for(s);
    if (ps.splits > 1 && wsl.ptr) {                 // cap the split count by the slab space
        const long long cap = wsl.bytes / (nk * 4);
        if (cap < 2) { p.ws = nullptr; }
        else {
            if (ps.splits > cap) ps = pixel_split(p.M, (int)cap);
            p.ws = wsl.ptr;
        }
    }
    float* det_dB = nullptr;
    if (sidlsg_det() && ps.splits > 1) {
        if (!p.ws || (p.dB && (p.N & 7))) {
            ps = pixel_split(p.M, 1); p.ws = nullptr;
        } else {
            det_dB = p.dB; p.dB = nullptr;
        }
    }
    const int splits = ps.splits;
    p.m_per_split = ps.mps;
    p.nsplits = splits;
    bool cf = false;
    if (v2 && MODE == 1 && !p.slow_gather && !p.ups && p.H == p.Ho * p.stride) {          // conditions of the constant-advance gather (wgrad_v2_body, fastc)
        const int hw = p.Ho * p.Wo, d_b = WG_MB / hw, d_rem = WG_MB - d_b * hw;
        const int d_wo = d_rem - (d_rem / p.Wo) * p.Wo;
        const unsigned long long rowb = (unsigned long long)p.Wd * p.lda * 2ull;
        cf = d_wo == 0 && (unsigned long long)p.a_bytes + rowb < 0x7fffffffull;
    }
    record_launch(!v2 ? SIDLSG_K_WGRAD_BF16 : sq160 ? SIDLSG_K_WGRAD_V2S : cf ? (tn == 160 ? SIDLSG_K_WGRAD_V2WF : SIDLSG_K_WGRAD_V2F)
                                            : tn == 160 ? SIDLSG_K_WGRAD_V2W : SIDLSG_K_WGRAD_V2,
                  tn, tk, MODE, -1, -1, splits, splits <= 1 ? SIDLSG_PART_ONE : p.ws ? SIDLSG_PART_SLABS : SIDLSG_PART_ATOMICS);
    if (splits > 1 && p.ws) record_followup(SIDLSG_FIN_WGRAD_REDUCE);
    if (det_dB) record_followup(SIDLSG_FIN_COLSUM);
    if (p.assign && splits > 1 && !p.ws) {         // fp32-atomic fallback (no slab space): the atomics need a zeroed target
        if (hipMemsetAsync(p.dW, 0, (size_t)nk * sizeof(float), s) != hipSuccess) return sidlsg_last_error();
    }
    if (v2) {
        const size_t lds = (size_t)wgrad_v2_lds(tn, tk);
        if (const int e = sq160 ? sidlsg_lds_limit<&wgrad_v2s_kernel>(lds) : cf && tn == 160 ? sidlsg_lds_limit<&wgrad_v2wf_kernel>(lds)
                        : cf ? sidlsg_lds_limit<&wgrad_v2f_kernel>(lds) : tn == 160 ? sidlsg_lds_limit<&wgrad_v2w_kernel<MODE>>(lds)
                        : sidlsg_lds_limit<&wgrad_v2_kernel<MODE>>(lds)) return e;
        if (sq160) SIDLSG_LAUNCH(wgrad_v2s_kernel, dim3(tiles * splits), dim3(NTHREADS), lds, s, p);
        else if (cf && tn == 160) SIDLSG_LAUNCH(wgrad_v2wf_kernel, dim3(tiles * splits), dim3(NTHREADS), lds, s, p);
        else if (cf) SIDLSG_LAUNCH(wgrad_v2f_kernel, dim3(tiles * splits), dim3(NTHREADS), lds, s, p);
        else if (tn == 160) SIDLSG_LAUNCH((wgrad_v2w_kernel<MODE>), dim3(tiles * splits), dim3(NTHREADS), lds, s, p);
        else SIDLSG_LAUNCH((wgrad_v2_kernel<MODE>), dim3(tiles * splits), dim3(NTHREADS), lds, s, p);
    } else
    SIDLSG_LAUNCH((wgrad_bf16_kernel<MODE>), dim3(tiles, splits), dim3(NTHREADS), 0, s, p);
    if (splits > 1 && p.ws)
        SIDLSG_LAUNCH(wgrad_reduce_kernel, dim3((unsigned)((nk / 4 + 256) / 256)), dim3(256), 0, s, p.ws, p.dW, (size_t)nk, splits, p.assign);
    if (det_dB) return sidlsg_colsum(p.dY, p.ldy, nullptr, det_dB, nullptr, 1, p.M, p.N, s);      // after the reduction: it reuses the workspace
    return sidlsg_last_error();
}

// Host side of the grouped dense weight gradient.  Every job must be one the 128 x 128 direct-to-LDS kernel takes (aligned operands);
// the split count is chosen for the GROUP: all jobs together should put ~512 blocks on the chip (whole rounds, like launch_wgrad's
// model): every job gets the same split count `want` = slots / (tiles of all jobs), limited by its own row count (>= 4 stages per split) and by
// what is left of the stream's workspace for its slabs.
static int launch_wgrad_group(WgradParams* jobs, int njobs, hipStream_t s, bool t160) {
    if (njobs < 1 || njobs > WG_GROUP) return SIDLSG_EINVAL;
    long long tiles[WG_GROUP], total_tiles = 0;
    for (int i = 0; i < njobs; i++) {
        const WgradParams& p = jobs[i];
        const bool aligned = !(p.N & 7) && !(p.K & 7) && !(p.ldy & 7) && !(p.lda & 7) && !(((uintptr_t)p.dY | (uintptr_t)p.A) & 15);
        if (!aligned || (t160 && (p.N % 160 || p.K % 160))) return SIDLSG_EINVAL;
        tiles[i] = t160 ? (long long)(p.N / 160) * (p.K / 160) : (long long)((p.N + 127) / 128) * ((p.K + WG_T - 1) / WG_T);
        total_tiles += tiles[i];
    }
    const Ws wsl = ws_for(s);
    static const int slots = sidlsg_env_int("SIDLSG_WGRAD_SLOTS", 512);
    int want = (int)std::max<long long>(1, slots / std::max<long long>(1, total_tiles));        // splits per job when all rows counts are equal
    WgradGroup g{};
    WgradReduceGroup rg{};
    g.njobs = njobs;
    int blocks = 0, rjobs = 0;
    unsigned rblocks = 0;
    long long ws_used = 0;
    float* det_dB[WG_GROUP] = {};
    for (int i = 0; i < njobs; i++) {
        WgradParams p = jobs[i];
        const int max_splits = (p.M + 4 * WG_MB - 1) / (4 * WG_MB);
        PixelSplit ps = pixel_split(p.M, std::min(std::min(want, 64), std::max(1, max_splits)));
        const long long nk = (long long)p.N * p.K;
        p.ws = nullptr;
        if (ps.splits > 1) {
            // slabs that do not fit what is left of the workspace: as many splits as do fit (launch_wgrad does the same), one only when not even two fit
            const long long fit = (wsl.ptr && !(nk & 3)) ? (wsl.bytes - ws_used) / (nk * 4) : 0;
            if (fit < ps.splits) ps = pixel_split(p.M, fit >= 2 ? (int)fit : 1);
        }
        const int splits = ps.splits;
        if (splits > 1) { p.ws = reinterpret_cast<float*>(reinterpret_cast<char*>(wsl.ptr) + ws_used); ws_used += ((long long)splits * nk * 4 + 255) / 256 * 256; }
        if (sidlsg_det() && splits > 1 && p.dB) { det_dB[i] = p.dB; p.dB = nullptr; }      // (see launch_wgrad)
        p.m_per_split = ps.mps;
        p.nsplits = splits;
        g.blk0[i] = blocks;
        p.bid0 = blocks;
        g.j[i] = p;
        blocks += (int)((tiles[i] * splits + 7) / 8 * 8);
        if (splits > 1) {
            rg.blk0[rjobs] = rblocks; rg.ws[rjobs] = p.ws; rg.dW[rjobs] = p.dW; rg.n4[rjobs] = (unsigned)(nk / 4);
            rg.splits[rjobs] = splits; rg.assign[rjobs] = p.assign;
            rblocks += (unsigned)((nk / 4 + 255) / 256);
            rjobs++;
        }
    }
    {
        int max_splits = 1;
        for (int i = 0; i < njobs; i++) max_splits = std::max(max_splits, g.j[i].nsplits);
        bool det_bias = false;
        for (int i = 0; i < njobs; i++) det_bias = det_bias || det_dB[i];
        record_launch(t160 ? SIDLSG_K_WGRAD_V2SG : SIDLSG_K_WGRAD_V2G, t160 ? 160 : 128, t160 ? 160 : WG_T, 0, -1, -1, max_splits,
                      rjobs ? SIDLSG_PART_SLABS : SIDLSG_PART_ONE);
        if (rjobs) record_followup(SIDLSG_FIN_WGRAD_REDUCE);
        if (det_bias) record_followup(SIDLSG_FIN_COLSUM);
    }
    g.blk0[njobs] = blocks;
    rg.njobs = rjobs; rg.blk0[rjobs] = rblocks;
    const size_t lds = (size_t)(t160 ? wgrad_v2_lds(160, 160) : wgrad_v2_lds(128, WG_T));
    if (const int e = t160 ? sidlsg_lds_limit<&wgrad_v2sg_kernel>(lds) : sidlsg_lds_limit<&wgrad_v2g_kernel>(lds)) return e;
    if (t160) SIDLSG_LAUNCH(wgrad_v2sg_kernel, dim3(blocks), dim3(NTHREADS), lds, s, g);
    else SIDLSG_LAUNCH(wgrad_v2g_kernel, dim3(blocks), dim3(NTHREADS), lds, s, g);
    if (rjobs) SIDLSG_LAUNCH(wgrad_reduce_g_kernel, dim3(rblocks), dim3(256), 0, s, rg);
    for (int i = 0; i < njobs; i++)
        if (det_dB[i])
            if (int e = sidlsg_colsum(jobs[i].dY, jobs[i].ldy, nullptr, det_dB[i], nullptr, 1, jobs[i].M, jobs[i].N, s)) return e;
    return sidlsg_last_error();
}

extern "C" {

// (diagnostic) resident blocks per CU of the weight-gradient kernels with their dynamic LDS: 0 = 128x128, 1 = 160x128, 2 = 160x160
int sidlsg_debug_wgrad_blocks_per_cu(int which) {
    int n = -1;
    const size_t lds = (size_t)wgrad_v2_lds(which ? 160 : 128, which == 2 ? 160 : WG_T);
    const void* f = which == 2 ? reinterpret_cast<const void*>(&wgrad_v2s_kernel)
                               : which ? reinterpret_cast<const void*>(&wgrad_v2w_kernel<0>) : reinterpret_cast<const void*>(&wgrad_v2_kernel<0>);
    (void)hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, f, NTHREADS, lds) != hipSuccess) return -1;
    return n;
}

// dW[N][K] += dY[M][N]^T A[M][K]   (dense: Linear / 1x1 conv weight gradient; fp32 accumulate)
static int wgrad_dense_impl(const void* dY, int ldy, const void* A, int lda, float* dW, float* dBias, int M, int N, int K, int assign, void* stream) {
    if (M <= 0 || N <= 0 || K <= 0 || (K & 7) || (lda & 7) || !dY || !A || !dW) return SIDLSG_EINVAL;
    WgradParams p{};
    p.dY = (const bf16*)dY; p.A = (const bf16*)A; p.dW = dW; p.dB = dBias; p.M = M; p.N = N; p.K = K; p.ldy = ldy; p.lda = lda; p.assign = assign;
    if (!range31(p.a_bytes, M, lda, K, 2) || !range31(p.y_bytes, M, ldy, N, 2)) return SIDLSG_EINVAL;
    SidlsgTraceScope ts(SIDLSG_FAM_WGRAD, 2.0 * M * (double)N * K, 2.0 * ((double)M * N + (double)M * K) + (assign ? 4.0 : 8.0) * N * K);      // dY, A read once; dW (read +) written (fp32)
    return launch_wgrad<0>(p, (hipStream_t)stream);
}
int sidlsg_wgrad_bf16(const void* dY, int ldy, const void* A, int lda, float* dW, float* dBias, int M, int N, int K, void* stream) {
    return wgrad_dense_impl(dY, ldy, A, lda, dW, dBias, M, N, K, 0, stream);
}
// dW = dY^T A (dBias still +=): for a gradient buffer whose previous contents are dead -- the fused optimizer leaves the weight
// gradients un-zeroed (sidlsg_adam_ema with zero_grad = 0 on those ranges) and the first weight gradient after it overwrites them,
// which saves the optimizer's 4 B / parameter of zero stores and this kernel's (or its reduction's) 4 B / parameter read of dW.
// Same summation order as the accumulating entry point on a zeroed dW: bit-identical results.
int sidlsg_wgrad_assign_bf16(const void* dY, int ldy, const void* A, int lda, float* dW, float* dBias, int M, int N, int K, void* stream) {
    return wgrad_dense_impl(dY, ldy, A, lda, dW, dBias, M, N, K, 1, stream);
}

// Several dense weight gradients as ONE launch (+ one slab-reduction launch): jobs = host array of njobs <= 8 records
//   { const void* dY; const void* A; float* dW; float* dBias; int ldy, lda, M, N, K, assign; int pad[2]; }      (64 bytes each)
// with the meaning of sidlsg_wgrad_bf16 / _assign_bf16 per record.  Every job must satisfy the alignment of the direct-to-LDS kernel
// (N, K, ldy, lda multiples of 8, 16-byte aligned operands), else EINVAL and nothing is launched.  Bit-identical per job to the single
// entry points wherever both choose the same split count; otherwise the fp32 summation order over pixels differs.
struct sidlsg_wgrad_job { const void* dY; const void* A; float* dW; float* dBias; int ldy, lda, M, N, K, assign; int pad[2]; };
static int wgrad_group_impl(const void* jobs, int njobs, void* stream, bool t160) {
    if (!jobs || njobs < 1 || njobs > WG_GROUP) return SIDLSG_EINVAL;
    const sidlsg_wgrad_job* in = (const sidlsg_wgrad_job*)jobs;
    WgradParams ps[WG_GROUP];
    double flop = 0, bytes = 0;
    for (int i = 0; i < njobs; i++) {
        const sidlsg_wgrad_job& q = in[i];
        if (q.M <= 0 || q.N <= 0 || q.K <= 0 || !q.dY || !q.A || !q.dW) return SIDLSG_EINVAL;
        WgradParams p{};
        p.dY = (const bf16*)q.dY; p.A = (const bf16*)q.A; p.dW = q.dW; p.dB = q.dBias; p.M = q.M; p.N = q.N; p.K = q.K; p.ldy = q.ldy; p.lda = q.lda;
        p.assign = q.assign;
        if (!range31(p.a_bytes, q.M, q.lda, q.K, 2) || !range31(p.y_bytes, q.M, q.ldy, q.N, 2)) return SIDLSG_EINVAL;
        ps[i] = p;
        flop += 2.0 * q.M * (double)q.N * q.K;
        bytes += 2.0 * ((double)q.M * q.N + (double)q.M * q.K) + (q.assign ? 4.0 : 8.0) * q.N * q.K;
    }
    SidlsgTraceScope ts(SIDLSG_FAM_WGRAD, flop, bytes);
    return launch_wgrad_group(ps, njobs, (hipStream_t)stream, t160);
}
int sidlsg_wgrad_group_bf16(const void* jobs, int njobs, void* stream) { return wgrad_group_impl(jobs, njobs, stream, false); }
// The same on 160 x 160 tiles: every job's N and K must be multiples of 160 (the q|k|v, FF-in and FF-out projections of a transformer block)
int sidlsg_wgrad_group160_bf16(const void* jobs, int njobs, void* stream) { return wgrad_group_impl(jobs, njobs, stream, true); }

// dW[Cout][3][3][Cin] += conv3x3 weight gradient (same geometry arguments as sidlsg_conv3x3_bf16)
static int wgrad_conv_impl(const void* dY, int ldy, const void* X, int ldx, float* dW, float* dBias, int B, int H, int Wd,
                           int Cin, int Cout, int stride, int ups, int assign, void* stream) {
    if ((stride != 1 && stride != 2) || (Cin & 7) || (ldx & 7) || !dY || !X || !dW) return SIDLSG_EINVAL;
    WgradParams p{};
    p.dY = (const bf16*)dY; p.A = (const bf16*)X; p.dW = dW; p.dB = dBias; p.ldy = ldy; p.lda = ldx; p.assign = assign;
    static const int slow_gather = !sidlsg_env_on("SIDLSG_WGRAD_CONV_FAST");      // A/B switch
    p.slow_gather = slow_gather;
    p.H = H; p.Wd = Wd; p.Cin = Cin; p.stride = stride; p.ups = ups;
    p.Ho = (H + 2 - 3) / stride + 1; p.Wo = (Wd + 2 - 3) / stride + 1;
    p.M = B * p.Ho * p.Wo; p.N = Cout; p.K = 9 * Cin;
    const int Hs = ups ? H / 2 : H, Ws = ups ? Wd / 2 : Wd;
    if (!range31(p.a_bytes, conv_src_pixels(B, H, Wd, ups), ldx, Cin, 2) || !range31(p.y_bytes, p.M, ldy, Cout, 2)) return SIDLSG_EINVAL;
    SidlsgTraceScope ts(SIDLSG_FAM_CONV_WGRAD, 2.0 * p.M * (double)p.N * p.K,
                        2.0 * ((double)p.M * p.N + (double)B * Hs * Ws * Cin) + (assign ? 4.0 : 8.0) * p.N * p.K);
    return launch_wgrad<1>(p, (hipStream_t)stream);
}
int sidlsg_conv3x3_wgrad_bf16(const void* dY, int ldy, const void* X, int ldx, float* dW, float* dBias, int B, int H, int Wd,
                              int Cin, int Cout, int stride, int ups, void* stream) {
    return wgrad_conv_impl(dY, ldy, X, ldx, dW, dBias, B, H, Wd, Cin, Cout, stride, ups, 0, stream);
}
int sidlsg_conv3x3_wgrad_assign_bf16(const void* dY, int ldy, const void* X, int ldx, float* dW, float* dBias, int B, int H, int Wd,
                                     int Cin, int Cout, int stride, int ups, void* stream) {
    return wgrad_conv_impl(dY, ldy, X, ldx, dW, dBias, B, H, Wd, Cin, Cout, stride, ups, 1, stream);
}

}  // extern "C"
