// e4m3 contractions of FROZEN networks for gfx950 (MI355X), on gemm_core.h's parameter block, loader conventions and epilogue:
//   gemm_fp8w_kernel<MODE>    e4m3 weights, bf16 activations converted in the loader (sidlsg_*_fp8w*)
//   gemm_mx8_kernel<MODE>     both operands e4m3 on the MX-scaled K = 128 MFMA (sidlsg_*_mx8*); its split-K launches finish through
//                             gemm.hip's gemm_finish_kernel (launch_gemm_finish)
//   quantize_fp8_rows_kernel, cast_fp8_kernel    weights -> e4m3 + per-row scale; activations -> e4m3 at unit scale
#include "gemm_core.h"

// ---------------------------------------------------------------------------------------------
// fp8-weight path (BASELINE.json configs[4]: "fp8 MFMA weights + bf16 accum"; no reference behaviour exists for it --
// SURVEY.md Appendix C -- so the contract is this file's): frozen networks (teacher, fake score under evaluation) keep
// their GEMM / conv weights as OCP e4m3 bytes with one fp32 scale per output channel (sidlsg_quantize_fp8_rows); the
// activations arrive as bf16, are converted to e4m3 in the loader (static unit scale, clamped to +-448 before the conversion: normalised
// activations sit well inside that range, the residual stream of real weights may not) and the contraction runs on v_mfma_f32_16x16x32_fp8_fp8 with fp32 accumulation;
// the epilogue multiplies by the channel scale.  Half the operand bytes through L2 / LDS; the non-scaled fp8 MFMA has
// the bf16 rate on gfx950 (only the MX block-scaled K=128 forms are faster), so this is a bandwidth, not a FLOP, lever.
// 128 x 128 x 64 tile, 4 waves (64 x 64 each), register-staged loads (the bf16 -> fp8 conversion needs registers), LDS
// rows of 64 bytes padded to 80 so the 8-byte fragment reads of a half-wave fall on distinct banks.
typedef long i64_t;
constexpr int F8_T = 128, F8_LD = 80;     // tile edge; LDS row stride in bytes

// (clamp_e4m3 / cvt4_fp8: common.h)

template <int MODE>   // 0 dense rows, 2 conv3x3 (any Cin % 8 == 0)
__global__ __launch_bounds__(NTHREADS, 2) void gemm_fp8w_kernel(GemmParams p) {
    __shared__ __attribute__((aligned(16))) unsigned char As[2][F8_T * F8_LD];
    __shared__ __attribute__((aligned(16))) unsigned char Ws[2][F8_T * F8_LD];
    const int tiles_n = (p.N + F8_T - 1) / F8_T;
    const int nblk = tiles_n * m_tiles_rt(p, F8_T);
    const int bid = xcd_contiguous((int)blockIdx.x, nblk);
    const int m0 = group_select<F8_T>(p, bid / tiles_n), n0 = (bid % tiles_n) * F8_T;      // (before the weight descriptor is built)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lg = lane >> 4;
    const int wm0 = (wave >> 1) * 64, wn0 = (wave & 1) * 64;
    const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16*>(p.A), 0, (int)p.a_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16*>(p.W), 0, (int)p.w_bytes, 0x00020000);
    const unsigned char* W8 = reinterpret_cast<const unsigned char*>(p.W);
    (void)W8;
    // A loader: 4 chunks of 8 bf16 per thread: chunk c = tid & 7 (k = c*8), rows r = (tid >> 3) + 32 i
    const int kc = tid & 7, r0 = tid >> 3;
    const int Hs = p.ups ? (p.H >> 1) : p.H, Wsrc = p.ups ? (p.Wd >> 1) : p.Wd;
    unsigned abase[4];
    int ahi[4], awi[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int m = m0 + r0 + 32 * i;
        const bool ok = m < p.M;
        if (MODE == 0) { abase[i] = ok ? (unsigned)m * (unsigned)p.lda * 2u : OOB; ahi[i] = awi[i] = 0; }
        else {
            const ConvRow cr = conv_row(p, m);
            abase[i] = (unsigned)cr.b * (unsigned)(Hs * Wsrc) * (unsigned)p.lda * 2u;
            ahi[i] = cr.hi(p, 1);
            awi[i] = cr.wi(p, 1);
        }
    }
    // W loader: fp8 rows of K bytes: 2 chunks of 16 bytes per thread: chunk c = tid & 3 (k = c*16), rows (tid >> 2) + 64 i
    const int wc = tid & 3, wr0 = tid >> 2;
    bf16x8 areg[4];
    u32x4 wreg[2];
    auto load_tile = [&](int kt) {
        const int k = kt * BK + kc * 8;
        const bool kok = k < p.K;
        int dh = 0, dw = 0, c = k;
        if (MODE != 0) { const int tap = k / p.Cin; c = k - tap * p.Cin; dh = tap / 3; dw = tap - dh * 3; }
#pragma unroll
        for (int i = 0; i < 4; i++) {
            unsigned off = OOB;
            if (kok && abase[i] != OOB) {
                if (MODE == 0) off = abase[i] + (unsigned)k * 2u;
                else {
                    int hi = ahi[i] + dh, wi = awi[i] + dw;
                    const bool ok = hi >= 0 && hi < p.H && wi >= 0 && wi < p.Wd;
                    if (p.ups) { hi >>= 1; wi >>= 1; }
                    if (ok) off = abase[i] + ((unsigned)(hi * Wsrc + wi) * (unsigned)p.lda + (unsigned)c) * 2u;
                }
            }
            areg[i] = buf_ld8(ra, off);
        }
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const int n = n0 + wr0 + 64 * i, kb = kt * BK + wc * 16;
            wreg[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rw, (n < p.N && kb < p.K) ? (unsigned)n * (unsigned)p.K + (unsigned)kb : OOB, 0, 0));
        }
    };
    auto store_tile = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const bf16x8 v = areg[i];
            u32x2 q = {cvt4_fp8(bf2f(v[0]), bf2f(v[1]), bf2f(v[2]), bf2f(v[3])), cvt4_fp8(bf2f(v[4]), bf2f(v[5]), bf2f(v[6]), bf2f(v[7]))};
            *reinterpret_cast<u32x2*>(&As[buf][(r0 + 32 * i) * F8_LD + kc * 8]) = q;
        }
#pragma unroll
        for (int i = 0; i < 2; i++) *reinterpret_cast<u32x4*>(&Ws[buf][(wr0 + 64 * i) * F8_LD + wc * 16]) = wreg[i];
    };
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    int wrow[4];
#pragma unroll
    for (int ni = 0; ni < 4; ni++) wrow[ni] = wn0 + 32 * (ni >> 1) + (li >> 2) * 8 + (ni & 1) * 4 + (li & 3);
    const int nk = (p.K + BK - 1) / BK;
    load_tile(0);
    store_tile(0);
    __syncthreads();
    for (int kt = 0; kt < nk; kt++) {
        const int buf = kt & 1;
        if (kt + 1 < nk) load_tile(kt + 1);
#pragma unroll
        for (int kk = 0; kk < 2; kk++) {
            i64_t fa[4], fw[4];
#pragma unroll
            for (int mi = 0; mi < 4; mi++) fa[mi] = *reinterpret_cast<const i64_t*>(&As[buf][(wm0 + mi * 16 + li) * F8_LD + kk * 32 + lg * 8]);
#pragma unroll
            for (int ni = 0; ni < 4; ni++) fw[ni] = *reinterpret_cast<const i64_t*>(&Ws[buf][wrow[ni] * F8_LD + kk * 32 + lg * 8]);
#pragma unroll
            for (int ni = 0; ni < 4; ni++)
#pragma unroll
                for (int mi = 0; mi < 4; mi++)
                    acc[ni][mi] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(fw[ni], fa[mi], acc[ni][mi], 0, 0, 0);
        }
        if (kt + 1 < nk) store_tile(buf ^ 1);
        __syncthreads();
    }
    // per-output-channel dequantisation scales, applied in place (lane (lg, li): channels n .. n+7 of each tile pair)
#pragma unroll
    for (int pr = 0; pr < 2; pr++) {
        const int n = n0 + wn0 + 32 * pr + lg * 8;
        float sc[8];
#pragma unroll
        for (int e = 0; e < 8; e++) sc[e] = (n + e < p.N) ? p.wscale[n + e] : 0.f;
#pragma unroll
        for (int mi = 0; mi < 4; mi++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                acc[2 * pr][mi][r] *= sc[r];
                acc[2 * pr + 1][mi][r] *= sc[4 + r];
            }
    }
    EpiPre<4> pre;
    epilogue_prefetch<4>(p, pre, n0 + wn0, lg);
    gemm_epilogue<4, 4>(p, acc, m0 + wm0, n0 + wn0, li, lg, pre);
}

// per-row e4m3 quantisation of a bf16 matrix [rows][cols] (cols % 8 == 0): scale[r] = max|x| / 448 (1 if the row is zero),
// q = cvt_fp8(x / scale).  One wave per row.
__global__ __launch_bounds__(256) void quantize_fp8_rows_kernel(const bf16* __restrict__ src, unsigned char* __restrict__ dst,
                                                                float* __restrict__ scale, int rows, int cols) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const bf16* s = src + (size_t)row * cols;
    float amax = 0.f;
    for (int c = lane * 8; c < cols; c += 512) {
        const bf16x8 v = ld8(s + c);
#pragma unroll
        for (int e = 0; e < 8; e++) amax = fmaxf(amax, fabsf(bf2f(v[e])));
    }
    amax = wave_max(amax);
    const float sc = amax > 0.f ? amax / 448.f : 1.f;
    const float inv = 1.f / sc;
    if (lane == 0) scale[row] = sc;
    for (int c = lane * 8; c < cols; c += 512) {
        const bf16x8 v = ld8(s + c);
        u32x2 q = {cvt4_fp8(bf2f(v[0]) * inv, bf2f(v[1]) * inv, bf2f(v[2]) * inv, bf2f(v[3]) * inv),
                   cvt4_fp8(bf2f(v[4]) * inv, bf2f(v[5]) * inv, bf2f(v[6]) * inv, bf2f(v[7]) * inv)};
        *reinterpret_cast<u32x2*>(dst + (size_t)row * cols + c) = q;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// MX-fp8 dense GEMM for FROZEN networks:  C[m][n] = wscale[n] * sum_k A8[m][k] * W8[n][k]  (+ the shared epilogue)
// with BOTH operands OCP e4m3 bytes (A8: activations the producing GroupNorm / LayerNorm kernel wrote as e4m3 at unit
// scale; W8 + wscale: sidlsg_quantize_fp8_rows) on v_mfma_scale_f32_16x16x128_f8f6f4 with unit E8M0 block scales -- the only
// 8-bit MFMA form that runs at twice the bf16 rate on gfx950 (tools/ubench/mfma_f8.hip: 4.27 vs 1.83 PFLOP/s register-only;
// the non-scaled 16x16x32 fp8 form of gemm_fp8w_kernel has the bf16 instruction rate).
// A K-tile of 128 e4m3 elements is byte-identical to gemm_v3_kernel's 64 bf16 elements: same 128 x 160 tile, 128-byte LDS
// rows, direct-to-LDS loader with one 32-bit offset per row, the same conflict-free swizzles and the same one-barrier
// schedule.  The MFMA wants 32 consecutive K bytes per lane and operand; which 32 is free as long as both operands agree, so
// lane group lg takes the 16-byte chunks lg and 4 + lg of its row -- exactly the two ds_read_b128 patterns of the bf16 kernel
// (chunks 2 lg, 2 lg + 1 would be 2-way bank conflicted with these swizzles).  Schedule per K-tile, halves by output column:
//   A: reads of the W fragments ni = 2..4 of the current tile; MFMAs ni = 0..1    C: vmcnt(0); s_barrier
//   D: reads of the next tile's A fragments + W fragments ni = 0..1; DMA of tile kt+2    E: MFMAs ni = 2..4
// Requires N % 160 == 0, K % 16 == 0, lda % 16 == 0, bf16 or fp32 output through the shared epilogue.
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef int i32x4v __attribute__((ext_vector_type(4)));

template <int MODE>      // 0: dense rows.  1: conv3x3, pad 1, stride 1, no upsampling, Cin % 16 == 0 (NHWC e4m3 image)
__global__ __launch_bounds__(NTHREADS, 2) void gemm_mx8_kernel(GemmParams p) {
    constexpr int BM = 128, BN = 160, MT = 4, NT = 5, KB = 128;      // KB: bytes (= e4m3 elements) per K-tile
    constexpr int STAGE = (BM + BN) * KB;                            // bytes
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tiles_n = p.N / BN, tiles_m = m_tiles_rt(p, BM);
    const int ntile = tiles_n * tiles_m;
    const int nk_all = MODE == 1 ? 9 * ((p.Cin + KB - 1) / KB) : (p.K + KB - 1) / KB;
    const int nsplit = p.kt_per_split ? (nk_all + p.kt_per_split - 1) / p.kt_per_split : 1;
    const int bid = xcd_contiguous((int)blockIdx.x, ntile * nsplit);
    const int split = bid / ntile;       // split-K (few-tile launches, see launch_gemm_mx8): fp32 slabs + gemm_finish_kernel
    int mt, nt;
    {
        const int t = bid - split * ntile;
        const int per_group = p.group_m * tiles_n;
        const int g = t / per_group, first_m = g * p.group_m;
        const int gm = min(p.group_m, tiles_m - first_m);
        const int in_g = t - g * per_group;
        mt = first_m + in_g % gm;
        nt = in_g / gm;
    }
    // grouped launch: the block's set (weights, scales, bias, row limit) is chosen here, before W8 and its descriptor are read off p
    const int m0 = group_select<BM>(p, mt), n0 = nt * BN;
    const unsigned char* A8 = reinterpret_cast<const unsigned char*>(p.A);
    const unsigned char* W8 = reinterpret_cast<const unsigned char*>(p.W);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm0 = (wave >> 1) * 64, wn0 = (wave & 1) * 80;
    const int li = lane & 15, lg = lane >> 4;
    const int lrow = lane >> 3, lslot = lane & 7;
    // conv: K-tiles in the order "channel chunk outer, tap inner" with the tap as a wave-uniform soffset against a buffer base one
    // row + one pixel below the image and a 9-bit halo mask per row (see gemm_v3_kernel).  A chunk is 128 channels of one tap;
    // when Cin is not a multiple of 128 (320: 128 + 128 + 64) the lanes whose 16 channels lie past Cin read zeros from A -- W's
    // over-read then meets zeros (it runs into the next tap's weights, finite numbers; past the matrix the buffer returns zeros).
    const unsigned tap_rs = (unsigned)p.Wd * (unsigned)p.lda, tap_ps = (unsigned)p.lda;
    const unsigned shift = MODE == 1 ? tap_rs + tap_ps : 0u;
    const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(A8) - shift, 0, (int)(p.a_bytes + shift), 0x00020000);
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(W8), 0, (int)p.w_bytes, 0x00020000);
    unsigned aoff[4], boff[5];
    unsigned cen[4], tmask[4], akb[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int r = wave * 32 + j * 8 + lrow;
        const int kcs = lslot ^ ((r >> 1) & 7);
        const int m = m0 + r;
        aoff[j] = m < p.M ? (unsigned)m * (unsigned)p.lda + kcs * 16u : OOB;
        cen[j] = tmask[j] = akb[j] = 0;
        if (MODE == 1) {
            const bool ok = m < p.M;
            const int mm = ok ? m : 0, hw = p.H * p.Wd;
            const int b = mm / hw, rem = mm - b * hw;
            const int ho = rem / p.Wd, wo = rem - ho * p.Wd;
            cen[j] = (unsigned)((b * p.H + ho) * p.Wd + wo) * (unsigned)p.lda + kcs * 16u;
            akb[j] = kcs * 16u;
            unsigned mk = 0;
#pragma unroll
            for (int tp = 0; tp < 9; tp++) {
                const int hi = ho - 1 + tp / 3, wi = wo - 1 + tp % 3;
                if (ok && hi >= 0 && hi < p.H && wi >= 0 && wi < p.Wd) mk |= 1u << tp;
            }
            tmask[j] = mk;
            aoff[j] = OOB;
        }
    }
#pragma unroll
    for (int j = 0; j < 5; j++) {
        const int r = (wave + 4 * j) * 8 + lrow;
        const int kcs = lslot ^ wsw(r);
        boff[j] = (unsigned)(n0 + r) * (unsigned)p.K + kcs * 16u;       // N % 160 == 0: every row exists
    }
    const int kt_begin = p.kt_per_split ? split * p.kt_per_split : 0;
    const int nk = p.kt_per_split ? min(nk_all, kt_begin + p.kt_per_split) : nk_all;
    auto issue = [&](int t, int buf, const int part = 0) {          // 9 buffer_load ... lds per wave (part 1: the 4 A pieces, 2: the 5 W pieces)
        char* sa = smem + buf * STAGE;
        char* sb = sa + BM * KB;
        if (MODE == 1) {
            const int cc = t / 9, tap = t - cc * 9;
            const int dh = tap / 3, dw = tap - dh * 3;
            const unsigned sa_off = (unsigned)cc * KB + dh * tap_rs + dw * tap_ps;
            const unsigned sw_off = (unsigned)(tap * p.Cin + cc * KB);
            const unsigned lim = (unsigned)(p.Cin - cc * KB), bit = 1u << tap;
            if (part != 2) {
#pragma unroll
                for (int j = 0; j < 4; j++)
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (lptr_t)(sa + (wave * 32 + j * 8) * KB), 16, ((tmask[j] & bit) && akb[j] < lim) ? cen[j] : OOB, sa_off, 0, 0);
            }
            if (part != 1) {
#pragma unroll
                for (int j = 0; j < 5; j++) __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (lptr_t)(sb + (wave + 4 * j) * 8 * KB), 16, boff[j], sw_off, 0, 0);
            }
            return;
        }
        const int k0 = t * KB;
        if (k0 + KB > p.K) {                    // ragged K tail: chunks past K read zeros
            if (part != 2) {
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int kcs = lslot ^ (((wave * 32 + j * 8 + lrow) >> 1) & 7);
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (lptr_t)(sa + (wave * 32 + j * 8) * KB), 16, (k0 + kcs * 16 < p.K) ? aoff[j] : OOB, k0, 0, 0);
                }
            }
            if (part != 1) {
#pragma unroll
                for (int j = 0; j < 5; j++) {
                    const int kcs = lslot ^ wsw((wave + 4 * j) * 8 + lrow);
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (lptr_t)(sb + (wave + 4 * j) * 8 * KB), 16, (k0 + kcs * 16 < p.K) ? boff[j] : OOB, k0, 0, 0);
                }
            }
            return;
        }
        if (part != 2) {
#pragma unroll
            for (int j = 0; j < 4; j++) __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (lptr_t)(sa + (wave * 32 + j * 8) * KB), 16, aoff[j], k0, 0, 0);
        }
        if (part != 1) {
#pragma unroll
            for (int j = 0; j < 5; j++) __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (lptr_t)(sb + (wave + 4 * j) * 8 * KB), 16, boff[j], k0, 0, 0);
        }
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
    auto frag = [&](const char* rowp, int sw) -> i32x8 {     // chunks lg and 4 + lg of the row (swizzled positions)
        const i32x4v lo = *reinterpret_cast<const i32x4v*>(rowp + ((lg ^ sw) << 4));
        const i32x4v hi = *reinterpret_cast<const i32x4v*>(rowp + (((4 + lg) ^ sw) << 4));
        return (i32x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    };
    auto read_a = [&](int buf, i32x8 (&fa)[MT]) {
        const char* a = smem + buf * STAGE;
#pragma unroll
        for (int mi = 0; mi < MT; mi++) {
            const int r = wm0 + mi * 16 + li;
            fa[mi] = frag(a + r * KB, (r >> 1) & 7);
        }
    };
    auto read_w = [&](int buf, int ni) -> i32x8 {
        const char* b = smem + buf * STAGE + BM * KB;
        const int r = wrow[ni];
        return frag(b + r * KB, wsw(r));
    };
    auto mfma_col = [&](const i32x8 (&fa)[MT], const i32x8& fw, int ni) {
#pragma unroll
        for (int mi = 0; mi < MT; mi++)
            acc[ni][mi] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fw, fa[mi], acc[ni][mi], 0, 0, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
    };
    // K loop: tile kt lives in buffer kt & 1.  Top of a tile: my DMA share of it has landed (vmcnt(0)), the barrier publishes
    // it and tells that every wave is done reading the other buffer, whose refill with tile kt+1 starts right away; the
    // fragment reads of the tile start behind the barrier (their latency is covered by the co-resident block's waves: the
    // double-buffered register version of gemm_v3_kernel's schedule needs two 32-register A-fragment sets and spilled).
    i32x8 fa[MT], fw01[2], fw24[3];
    issue(kt_begin, 0);
    for (int kt = kt_begin; kt < nk; kt++) {
        const int buf = (kt - kt_begin) & 1;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
#if SIDLSG_MX8_SPREAD_DMA
        // fragment reads first; the 9 DMA pieces of the next tile are issued in two groups BETWEEN MFMA columns (a piece costs
        // the wave 60-185 cycles of issue: behind queued MFMAs that time is covered, in front of the reads it is not)
        const bool more = kt + 1 < nk;
        read_a(buf, fa);
        fw01[0] = read_w(buf, 0);
        fw01[1] = read_w(buf, 1);
        fw24[0] = read_w(buf, 2);
        fw24[1] = read_w(buf, 3);
        fw24[2] = read_w(buf, 4);
        mfma_col(fa, fw01[0], 0);
        __builtin_amdgcn_sched_barrier(0);
        if (more) issue(kt + 1, buf ^ 1, 1);
        __builtin_amdgcn_sched_barrier(0);
        mfma_col(fa, fw01[1], 1);
        mfma_col(fa, fw24[0], 2);
        __builtin_amdgcn_sched_barrier(0);
        if (more) issue(kt + 1, buf ^ 1, 2);
        __builtin_amdgcn_sched_barrier(0);
        mfma_col(fa, fw24[1], 3);
        mfma_col(fa, fw24[2], 4);
#else
        if (kt + 1 < nk) issue(kt + 1, buf ^ 1);
        read_a(buf, fa);
        fw01[0] = read_w(buf, 0);
        fw01[1] = read_w(buf, 1);
        fw24[0] = read_w(buf, 2);
        fw24[1] = read_w(buf, 3);
        fw24[2] = read_w(buf, 4);
        mfma_col(fa, fw01[0], 0);
        mfma_col(fa, fw01[1], 1);
        mfma_col(fa, fw24[0], 2);
        mfma_col(fa, fw24[1], 3);
        mfma_col(fa, fw24[2], 4);
#endif
    }
    if (p.kt_per_split) {                // partial sums (already scaled per channel) -> this split's fp32 slab
#pragma unroll
        for (int ni = 0; ni < NT; ni++) {
            const bool paired = (ni | 1) < NT;
            const int nb = n0 + wn0 + (paired ? 32 * (ni >> 1) + lg * 8 + (ni & 1) * 4 : 16 * ni + lg * 4);
            const f32x4 sc = *reinterpret_cast<const f32x4*>(p.wscale + nb);
#pragma unroll
            for (int mi = 0; mi < MT; mi++) {
                const int m = m0 + wm0 + mi * 16 + li;
                if (m < p.M) *reinterpret_cast<f32x4*>(p.ws + ((size_t)split * p.Mtot + m) * p.N + nb) = acc[ni][mi] * sc;
            }
        }
        return;
    }
    // (the bias is fetched here, not before the loop as in gemm_v3_kernel: its 24 registers would spill the two A-fragment sets)
    EpiPre<NT> pre;
    epilogue_prefetch<NT>(p, pre, n0 + wn0, lg);
    // per-output-channel dequantisation scale (accumulator layout: see gemm_v3_kernel's split-K store)
#pragma unroll
    for (int ni = 0; ni < NT; ni++) {
        const bool paired = (ni | 1) < NT;
        const int nb = n0 + wn0 + (paired ? 32 * (ni >> 1) + lg * 8 + (ni & 1) * 4 : 16 * ni + lg * 4);
        const f32x4 sc = *reinterpret_cast<const f32x4*>(p.wscale + nb);
#pragma unroll
        for (int mi = 0; mi < MT; mi++) acc[ni][mi] *= sc;
    }
    if (!(p.flags & (F_OUT_F32 | F_ACCUM))) {
        constexpr int LDR = BN + 8;
        bf16* ring = reinterpret_cast<bf16*>(smem);
        __syncthreads();
        gemm_epilogue<MT, NT>(p, acc, m0 + wm0, n0 + wn0, li, lg, pre, ring, m0, n0, LDR);
        __syncthreads();
        gemm_store_rows<BM, BN>(p, ring, m0, n0, LDR, tid);
        return;
    }
    gemm_epilogue<MT, NT, false>(p, acc, m0 + wm0, n0 + wn0, li, lg, pre);
}

template <int MODE>
static int launch_gemm_mx8(const GemmParams& p, hipStream_t s) {
    const int tiles = m_tiles_rt(p, 128) * (p.N / 160);
    const size_t lds = (size_t)2 * (128 + 160) * 128;
    GemmParams q = p;
    q.group_m = 4;
    q.Mtot = p.M;            // row count of a split-K slab (a block of a grouped launch narrows its own M)
    // few tiles (8x8 / 16x16 stages) and a long contraction: split K so that ~512 blocks exist (as gemm_v3_kernel does); the k-tiles
    // are 128 elements here, so half as many are required: 16 to split at all, 4 per split
    const int nk = MODE == 1 ? 9 * ((p.Cin + 127) / 128) : (p.K + 127) / 128;
    const Ws w = ws_for(s);
    int splits = splitk_splits(tiles, nk, (long long)p.M * p.N, w, 16, 4);
    if (splits > 1) {
        q.kt_per_split = (nk + splits - 1) / splits;
        q.ws = w.ptr;
        splits = (nk + q.kt_per_split - 1) / q.kt_per_split;
    }
    record_launch(SIDLSG_K_GEMM_MX8, 128, 160, MODE, -1, -1, splits, record_partial(splits));
    if (splits > 1) record_followup(SIDLSG_FIN_GEMM);
    if (const int e = sidlsg_lds_limit<&gemm_mx8_kernel<MODE>>(lds)) return e;
    SIDLSG_LAUNCH((gemm_mx8_kernel<MODE>), dim3(tiles * splits), dim3(NTHREADS), lds, s, q);
    if (splits > 1) launch_gemm_finish(q, splits, s);
    return sidlsg_last_error();
}

extern "C" {

// ---- fp8-weight contractions (see gemm_fp8w_kernel).  W8: e4m3 bytes [N][K]; wscale: fp32 [N].  K % 16 == 0.
int sidlsg_quantize_fp8_rows(const void* src_bf16, void* dst_fp8, float* scale, int rows, int cols, void* stream) {
    if (rows <= 0 || cols <= 0 || (cols & 7) || !src_bf16 || !dst_fp8 || !scale) return SIDLSG_EINVAL;
    SIDLSG_LAUNCH(quantize_fp8_rows_kernel, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, (const bf16*)src_bf16,
                       (unsigned char*)dst_fp8, scale, rows, cols);
    return sidlsg_last_error();
}

static int gemm_fp8w_impl(bool g2, const void* A, int lda, const void* W8, const float* wscale, const void* W8_1, const float* wscale1, void* C,
                          int ldc, const float* bias, const float* bias1, const void* res, int ldres, const float* rowvec, int ld_rowvec,
                          int rows_per_batch, int M, int N, int K, float alpha, int flags, void* stream) {
    if (g2 && (!wscale1 || !group2_args_ok(M, W8_1, bias, bias1))) return SIDLSG_EINVAL;
    GemmParams p = dense_params(A, lda, W8, C, ldc, bias, res, ldres, rowvec, ld_rowvec, rows_per_batch, M, N, K, alpha, flags);
    p.wscale = wscale;
    if (int e = check_common(p)) return e;
    if ((K & 15) || !wscale) return SIDLSG_EINVAL;
    if (!range31(p.a_bytes, M, lda, K, 2) || !range31(p.w_bytes, N, K, K, 1)) return SIDLSG_EINVAL;
    set_group2(p, g2, W8_1, wscale1, bias1);
    if (int e = check_epilogue(p)) return e;
    const int tiles = m_tiles_rt(p, F8_T) * ((N + F8_T - 1) / F8_T);
    record_launch(SIDLSG_K_GEMM_FP8W, F8_T, F8_T, 0, -1, -1, 1, SIDLSG_PART_ONE);
    SIDLSG_LAUNCH((gemm_fp8w_kernel<0>), dim3(tiles), dim3(NTHREADS), 0, (hipStream_t)stream, p);
    return sidlsg_last_error();
}
int sidlsg_gemm_fp8w(const void* A, int lda, const void* W8, const float* wscale, void* C, int ldc, const float* bias, const void* res,
                     int ldres, const float* rowvec, int ld_rowvec, int rows_per_batch, int M, int N, int K, float alpha,
                     int flags, void* stream) {
    return gemm_fp8w_impl(false, A, lda, W8, wscale, nullptr, nullptr, C, ldc, bias, nullptr, res, ldres, rowvec, ld_rowvec, rows_per_batch, M, N, K,
                          alpha, flags, stream);
}
int sidlsg_gemm_fp8w_g2(const void* A, int lda, const void* W8, const float* wscale, const void* W8_1, const float* wscale1, void* C, int ldc,
                        const float* bias, const float* bias1, const void* res, int ldres, const float* rowvec, int ld_rowvec,
                        int rows_per_batch, int M, int N, int K, float alpha, int flags, void* stream) {
    return gemm_fp8w_impl(true, A, lda, W8, wscale, W8_1, wscale1, C, ldc, bias, bias1, res, ldres, rowvec, ld_rowvec, rows_per_batch, M, N, K,
                          alpha, flags, stream);
}

static int gemm_mx8_impl(bool g2, const void* A8, int lda, const void* W8, const float* wscale, const void* W8_1, const float* wscale1, void* C,
                         int ldc, const float* bias, const float* bias1, const void* res, int ldres, const float* rowvec, int ld_rowvec,
                         int rows_per_batch, int M, int N, int K, float alpha, int flags, void* stream) {
    if (g2 && (!wscale1 || !group2_args_ok(M, W8_1, bias, bias1))) return SIDLSG_EINVAL;
    if (M <= 0 || N <= 0 || K <= 0 || !A8 || !W8 || !C || !wscale) return SIDLSG_EINVAL;
    if ((K & 15) || (lda & 15) || (N % 160) || lda < K) return SIDLSG_EINVAL;
    if (rowvec && rows_per_batch <= 0) return SIDLSG_EINVAL;
    if ((flags & F_ACCUM) && !(flags & F_OUT_F32)) return SIDLSG_EINVAL;
    GemmParams p = dense_params(A8, lda, W8, C, ldc, bias, res, ldres, rowvec, ld_rowvec, rows_per_batch, M, N, K, alpha, flags);
    p.wscale = wscale;
    if (!range31(p.a_bytes, M, lda, K, 1) || !range31(p.w_bytes, N, K, K, 1)) return SIDLSG_EINVAL;      // extents in bytes of e4m3
    set_group2(p, g2, W8_1, wscale1, bias1);
    if (int e = check_epilogue(p)) return e;
    SidlsgTraceScope ts(SIDLSG_FAM_GEMM, 2.0 * p.M * (double)p.N * p.K);
    return launch_gemm_mx8<0>(p, (hipStream_t)stream);
}
int sidlsg_gemm_mx8(const void* A8, int lda, const void* W8, const float* wscale, void* C, int ldc, const float* bias, const void* res,
                    int ldres, const float* rowvec, int ld_rowvec, int rows_per_batch, int M, int N, int K, float alpha,
                    int flags, void* stream) {
    return gemm_mx8_impl(false, A8, lda, W8, wscale, nullptr, nullptr, C, ldc, bias, nullptr, res, ldres, rowvec, ld_rowvec, rows_per_batch, M, N, K,
                         alpha, flags, stream);
}
int sidlsg_gemm_mx8_g2(const void* A8, int lda, const void* W8, const float* wscale, const void* W8_1, const float* wscale1, void* C, int ldc,
                       const float* bias, const float* bias1, const void* res, int ldres, const float* rowvec, int ld_rowvec,
                       int rows_per_batch, int M, int N, int K, float alpha, int flags, void* stream) {
    return gemm_mx8_impl(true, A8, lda, W8, wscale, W8_1, wscale1, C, ldc, bias, bias1, res, ldres, rowvec, ld_rowvec, rows_per_batch, M, N, K,
                         alpha, flags, stream);
}

static int conv3x3_mx8_impl(bool g2, const void* X8, int ldx, const void* W8, const float* wscale, const void* W8_1, const float* wscale1,
                            void* Y, int ldc, const float* bias, const float* bias1, const void* res, int ldres, const float* rowvec,
                            int ld_rowvec, int B, int H, int Wd, int Cin, int Cout, float alpha, int flags, void* stream) {
    if (g2 && (!wscale1 || !group2_args_ok(B, W8_1, bias, bias1))) return SIDLSG_EINVAL;
    if (B <= 0 || H <= 0 || Wd <= 0 || Cin <= 0 || Cout <= 0 || !X8 || !W8 || !Y || !wscale) return SIDLSG_EINVAL;
    if ((Cin & 15) || (ldx & 15) || (Cout % 160) || ldx < Cin) return SIDLSG_EINVAL;
    if ((flags & F_ACCUM) && !(flags & F_OUT_F32)) return SIDLSG_EINVAL;
    GemmParams p = conv_params(X8, ldx, W8, Y, ldc, bias, res, ldres, rowvec, ld_rowvec, B, H, Wd, Cin, Cout, 1, 0, alpha, flags);
    p.wscale = wscale;
    // the tap offsets reach (Wd + 1) pixels past a row's own: the check counts them, the descriptor range does not
    if (!range31(p.a_bytes, conv_src_pixels(B, H, Wd, 0), ldx, Cin, 1, (unsigned long long)(Wd + 1) * ldx) || !range31(p.w_bytes, 9ull * Cout, Cin, Cin, 1))
        return SIDLSG_EINVAL;
    set_group2(p, g2, W8_1, wscale1, bias1);
    if (int e = check_epilogue(p)) return e;
    SidlsgTraceScope ts(SIDLSG_FAM_CONV, 2.0 * p.M * (double)p.N * p.K);
    return launch_gemm_mx8<1>(p, (hipStream_t)stream);
}
int sidlsg_conv3x3_mx8(const void* X8, int ldx, const void* W8, const float* wscale, void* Y, int ldc, const float* bias, const void* res,
                       int ldres, const float* rowvec, int ld_rowvec, int B, int H, int Wd, int Cin, int Cout, float alpha, int flags,
                       void* stream) {
    return conv3x3_mx8_impl(false, X8, ldx, W8, wscale, nullptr, nullptr, Y, ldc, bias, nullptr, res, ldres, rowvec, ld_rowvec, B, H, Wd, Cin, Cout,
                            alpha, flags, stream);
}
int sidlsg_conv3x3_mx8_g2(const void* X8, int ldx, const void* W8, const float* wscale, const void* W8_1, const float* wscale1, void* Y, int ldc,
                          const float* bias, const float* bias1, const void* res, int ldres, const float* rowvec, int ld_rowvec, int B, int H,
                          int Wd, int Cin, int Cout, float alpha, int flags, void* stream) {
    return conv3x3_mx8_impl(true, X8, ldx, W8, wscale, W8_1, wscale1, Y, ldc, bias, bias1, res, ldres, rowvec, ld_rowvec, B, H, Wd, Cin, Cout,
                            alpha, flags, stream);
}

__global__ __launch_bounds__(256) void cast_fp8_kernel(const bf16* __restrict__ src, unsigned char* __restrict__ dst, size_t n8) {
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += stride) {
        const bf16x8 v = *reinterpret_cast<const bf16x8*>(src + i * 8);
        u32x2 q = {cvt4_fp8(bf2f(v[0]), bf2f(v[1]), bf2f(v[2]), bf2f(v[3])), cvt4_fp8(bf2f(v[4]), bf2f(v[5]), bf2f(v[6]), bf2f(v[7]))};
        *reinterpret_cast<u32x2*>(dst + i * 8) = q;
    }
}
int sidlsg_cast_fp8(const void* src_bf16, void* dst_fp8, long long n, void* stream) {
    if (!src_bf16 || !dst_fp8 || n <= 0 || (n & 7)) return SIDLSG_EINVAL;
    const size_t n8 = (size_t)n / 8;
    size_t blocks = (n8 + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;
    SIDLSG_LAUNCH(cast_fp8_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const bf16*)src_bf16, (unsigned char*)dst_fp8, n8);
    return sidlsg_last_error();
}

static int conv3x3_fp8w_impl(bool g2, const void* X, int ldx, const void* W8, const float* wscale, const void* W8_1, const float* wscale1,
                             void* Y, int ldc, const float* bias, const float* bias1, const void* res, int ldres, const float* rowvec,
                             int ld_rowvec, int B, int H, int Wd, int Cin, int Cout, int stride, int ups, float alpha, int flags,
                             void* stream) {
    if (g2 && (!wscale1 || !group2_args_ok(B, W8_1, bias, bias1))) return SIDLSG_EINVAL;
    if ((stride != 1 && stride != 2) || (Cin & 15) || !wscale) return SIDLSG_EINVAL;
    if (ups && ((H | Wd) & 1)) return SIDLSG_EINVAL;
    GemmParams p = conv_params(X, ldx, W8, Y, ldc, bias, res, ldres, rowvec, ld_rowvec, B, H, Wd, Cin, Cout, stride, ups, alpha, flags);
    p.wscale = wscale;
    if (int e = check_common(p)) return e;
    if (!range31(p.a_bytes, conv_src_pixels(B, H, Wd, ups), ldx, Cin, 2) || !range31(p.w_bytes, 9ull * Cout, Cin, Cin, 1)) return SIDLSG_EINVAL;
    set_group2(p, g2, W8_1, wscale1, bias1);
    if (int e = check_epilogue(p)) return e;
    const int tiles = m_tiles_rt(p, F8_T) * ((p.N + F8_T - 1) / F8_T);
    record_launch(SIDLSG_K_GEMM_FP8W, F8_T, F8_T, 2, -1, -1, 1, SIDLSG_PART_ONE);
    SIDLSG_LAUNCH((gemm_fp8w_kernel<2>), dim3(tiles), dim3(NTHREADS), 0, (hipStream_t)stream, p);
    return sidlsg_last_error();
}
int sidlsg_conv3x3_fp8w(const void* X, int ldx, const void* W8, const float* wscale, void* Y, int ldc, const float* bias,
                        const void* res, int ldres, const float* rowvec, int ld_rowvec, int B, int H, int Wd, int Cin, int Cout,
                        int stride, int ups, float alpha, int flags, void* stream) {
    return conv3x3_fp8w_impl(false, X, ldx, W8, wscale, nullptr, nullptr, Y, ldc, bias, nullptr, res, ldres, rowvec, ld_rowvec, B, H, Wd, Cin, Cout,
                             stride, ups, alpha, flags, stream);
}
int sidlsg_conv3x3_fp8w_g2(const void* X, int ldx, const void* W8, const float* wscale, const void* W8_1, const float* wscale1, void* Y, int ldc,
                           const float* bias, const float* bias1, const void* res, int ldres, const float* rowvec, int ld_rowvec, int B, int H,
                           int Wd, int Cin, int Cout, int stride, int ups, float alpha, int flags, void* stream) {
    return conv3x3_fp8w_impl(true, X, ldx, W8, wscale, W8_1, wscale1, Y, ldc, bias, bias1, res, ldres, rowvec, ld_rowvec, B, H, Wd, Cin, Cout,
                             stride, ups, alpha, flags, stream);
}

}  // extern "C"
