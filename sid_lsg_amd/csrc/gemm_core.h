// What the contraction units share: gemm.hip (bf16 forward), gemm_fp8.hip (e4m3 forward) and wgrad.hip (weight gradients), and the
// library state they reach in state.hip.  The parameter block, the common tiling constants, the epilogue family, the direct-to-LDS
// helpers and the measurement switches (device side); the parameter builders, the operand contract and the dispatch record (host side).
#pragma once
#include "common.h"
#include "../../include/sidlsg_hip.h"      // the kernel ids of the dispatch record (and a compile-time check of the C ABI against its definitions)
#include <stdlib.h>
#include <algorithm>
#include <type_traits>

struct GemmParams {
    const bf16* A;        // dense: [M][lda]; conv: NHWC image [B][Hs][Ws][ldx]
    const bf16* W;        // [N][K] row-major (K contiguous)
    void* C;              // [M][ldc] bf16 (or fp32 when OUT_F32)
    const float* bias;    // [N] or null
    const bf16* res;      // [M][ldres] or null
    const float* rowvec;  // [M/rows_per_batch][ldrv] or null (time-embedding broadcast)
    int ldrv;
    int M, N, K;
    int lda, ldc, ldres;
    int rows_per_batch;
    // conv3x3 (pad 1): virtual input H x Wd (after optional nearest x2 upsample), Cin channels
    int H, Wd, Cin, Ho, Wo, stride, ups;
    float alpha;
    int flags;
    unsigned a_bytes, w_bytes;   // sizes of the A / W allocations seen by the kernel (< 2 GiB)
    int kt_per_split;            // split-K: K-tiles per split (0 = no split)
    int group_m;                 // v3: m-tiles per group of the logical tile order (see gemm_v3_kernel)
    float* ws;                   // split-K: fp32 [splits][M][N] partial-sum slabs
    const float* wscale;         // fp8-weight path: per-output-channel dequantisation scale [N] (else null)
    // grouped launch (sidlsg_*_g2: two networks of identical shape evaluated on one stacked activation matrix): rows [0, Mg) are
    // contracted with (W, bias), rows [Mg, M) with (W1, bias1).  Mg = 0: ordinary launch.  Mtot: row count of a split-K slab
    // (= M; kept separately because a block narrows its M to its own set's row range, see group_select)
    const bf16* W1;
    const float* bias1;
    const float* wscale1;        // fp8-weight path: the second set's dequantisation scales (sidlsg_*_mx8_g2 / _fp8w_g2)
    int Mg, Mtot;
    // fused GEGLU (sidlsg_gemm_geglu_bf16: the transformer's FF-in projection): geglu = F = N / 2 > 0 -> an output tile holds 80
    // features of the "a" half (rows [80 t, +80) of W) and the SAME 80 features of the gate half (rows [F + 80 t, +80)), the
    // epilogue writes h (natural column order, C may be null) and Y[m][f] = a * gelu(g)
    bf16* Y;
    int ldy, geglu;
    // fused GEGLU BACKWARD (sidlsg_gemm_geglu_bwd_bf16: the data gradient of the FF-out projection): geglu_bwd = F > 0 -> the output
    // tile is dy[:, n0 .. n0 + 160) = dOut W2 (never stored); the epilogue reads h[:, n] / h[:, F + n] from Hin and writes
    // dH[:, n] = dy * gelu(g), dH[:, F + n] = dy * a * gelu'(g) to Y (both [M][ldy], ldy >= 2 F)
    const bf16* Hin;
    int geglu_bwd;
};

// m-tiles of a launch: each set of a grouped launch starts on a tile boundary of its own (Mg need not be a multiple of BM)
__host__ __device__ inline int m_tiles_rt(const GemmParams& p, int bm) { return p.Mg ? 2 * ((p.Mg + bm - 1) / bm) : (p.M + bm - 1) / bm; }
// the block's set: rewrites p (a by-value kernel argument: plain scalar registers) to that set's weights, bias and row limit
// and returns the block's first row.  Everything downstream (loader range checks, epilogue, stores) keeps using p unchanged.
template <int BM>
__device__ __forceinline__ int group_select(GemmParams& p, int mt) {
    if (!p.Mg) return mt * BM;
    const int tg = (p.Mg + BM - 1) / BM;
    if (mt >= tg) { p.W = p.W1; p.bias = p.bias1; p.wscale = p.wscale1; return p.Mg + (mt - tg) * BM; }
    p.M = p.Mg;
    return mt * BM;
}

enum { F_OUT_F32 = 1, F_SILU = 2, F_ACCUM = 4 };

constexpr int BK = 64;
constexpr int NTHREADS = 256;
constexpr unsigned OOB = 0x80000000u;   // any offset >= 2 GiB is out of range for our buffers -> load returns 0

DEVFN bf16x8 buf_ld8(__amdgpu_buffer_rsrc_t r, unsigned off) {
    return __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0));
}

// MODE 0: dense rows.  MODE 1: conv3x3 with Cin % 64 == 0 (a K-tile lies inside one tap).  MODE 2: conv3x3, any Cin % 8 == 0.
// Shared epilogue: lane (lg, li) holds, for pixel row m = mbase + mi*16 + li, 8 (or 4) consecutive channels per tile pair.
//
// Every global load of the epilogue is issued BEFORE the first store.  C is not __restrict__, so a load that follows a store
// in program order stays behind it: the earlier form (load bias / rowvec / residual, add, store, per 16-row block) made
// MT = 4 dependent round trips through a memory system that the co-resident blocks' tile DMAs keep saturated -- 5.5 us per
// 128 x 160 tile in the phase trace of tools/ab/gemm_trace.py, as long as the whole K loop of a K = 320 GEMM.  The bias
// (a function of the column only) can be fetched before the K loop (epilogue_prefetch) and costs nothing at all.
template <int NT>
struct EpiPre {
    float b[(NT + 1) / 2][8];
};

template <int NT>
DEVFN void epilogue_prefetch(const GemmParams& p, EpiPre<NT>& pre, int nbase, int lg) {
#pragma unroll
    for (int pr = 0; pr < (NT + 1) / 2; pr++) {
        const bool paired = (2 * pr + 1) < NT;
        const int cnt = paired ? 8 : 4;
        const int n = nbase + 32 * pr + lg * cnt;
#pragma unroll
        for (int e = 0; e < 8; e++) pre.b[pr][e] = 0.f;
        if (p.bias && (p.N & 7) == 0 && n < p.N) {
            const f32x4 b0 = *reinterpret_cast<const f32x4*>(p.bias + n);
            pre.b[pr][0] = b0[0]; pre.b[pr][1] = b0[1]; pre.b[pr][2] = b0[2]; pre.b[pr][3] = b0[3];
            if (paired) {
                const f32x4 b1 = *reinterpret_cast<const f32x4*>(p.bias + n + 4);
                pre.b[pr][4] = b1[0]; pre.b[pr][5] = b1[1]; pre.b[pr][6] = b1[2]; pre.b[pr][7] = b1[3];
            }
        }
    }
}

// stage != nullptr (bf16 outputs, N % 8 == 0): the finished values go to an LDS image of the block's output tile
// (row stride ldr elements, origin (tm0, tn0)) instead of global memory; gemm_store_rows then writes it out row-major.
//
// CODE SIZE is a first-order cost here.  One fully unrolled epilogue that tests every flag per 8-channel group (SiLU with its
// exp, fp32 / accumulate outputs, ragged N, residual, row vector) made gemm_v3_kernel 113 KB of code -- 97 KB of it epilogue --
// against a 64 KB instruction cache shared by two CUs whose four resident blocks are all in different phases.  The phase
// trace (tools/ab/gemm_trace.py) showed the epilogue of one 128 x 160 tile taking 5.5 - 7.3 us, as long as the whole K loop
// of a K = 320 GEMM, and 1.5 us with a bias-only build: the time was instruction fetch through a memory system that the
// tile DMAs keep saturated.  Hence: the feature set is decided ONCE per call (FEAT, uniform branch) and each hot
// combination (bf16 output, N % 8 == 0, no activation: bias only / + residual / + row vector) is its own compact
// straight-line instantiation; everything else takes the generic instantiation (FEAT 4, flags read at run time).
template <int MT, int NT, int FEAT>      // FEAT: 0 bias only, 1 + residual, 2 + row vector, 4 generic
DEVFN void epilogue_rows8(const GemmParams& p, f32x4 (&acc)[NT][MT], int mbase, int nbase, int li, int lg,
                          const EpiPre<NT>& pre, bf16* stage, int tm0, int tn0, int ldr) {
    constexpr int PR = (NT + 1) / 2;
    constexpr bool GENERIC = (FEAT & 4) != 0;
    const bool has_res = GENERIC ? p.res != nullptr : (FEAT & 1) != 0;
    const bool has_rv = GENERIC ? p.rowvec != nullptr : (FEAT & 2) != 0;
    const int flags = GENERIC ? p.flags : 0;
    // rowvec (one vector per batch image): the 16*MT <= 64 rows of this wave lie in at most two images when an image has
    // >= 64 rows (always on the SD path: 8 x 8 latents at the coarsest level) -> two vectors, selected per row
    f32x4 rvv[2][PR][2];
    bf16x8 rsv[MT][PR];
    const int img0 = (mbase < p.M ? mbase : 0) / p.rows_per_batch;
    const bool rv_two = has_rv && (!GENERIC || p.rows_per_batch >= 16 * MT);
    if (rv_two) {
        const int last = (min(mbase + 16 * MT, p.M) - 1) / p.rows_per_batch;
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const float* rv = p.rowvec + (size_t)(h ? max(last, img0) : img0) * p.ldrv;
#pragma unroll
            for (int pr = 0; pr < PR; pr++) {
                const bool paired = (2 * pr + 1) < NT;
                const int n = nbase + 32 * pr + lg * (paired ? 8 : 4);
                rvv[h][pr][0] = rvv[h][pr][1] = (f32x4){0.f, 0.f, 0.f, 0.f};
                if (mbase < p.M && n < p.N) {
                    rvv[h][pr][0] = *reinterpret_cast<const f32x4*>(rv + n);
                    if (paired) rvv[h][pr][1] = *reinterpret_cast<const f32x4*>(rv + n + 4);
                }
            }
        }
    }
    if (has_res) {
#pragma unroll
        for (int mi = 0; mi < MT; mi++) {
            const int m = mbase + mi * 16 + li;
#pragma unroll
            for (int pr = 0; pr < PR; pr++) {
                const bool paired = (2 * pr + 1) < NT;
                const int n = nbase + 32 * pr + lg * (paired ? 8 : 4);
                rsv[mi][pr] = zero8();
                if (m < p.M && n < p.N) {
                    const bf16* rp = p.res + (size_t)m * p.ldres + n;
                    if (paired) rsv[mi][pr] = ld8(rp);
                    else {
                        const bf16x4 t = *reinterpret_cast<const bf16x4*>(rp);
                        rsv[mi][pr][0] = t[0]; rsv[mi][pr][1] = t[1]; rsv[mi][pr][2] = t[2]; rsv[mi][pr][3] = t[3];
                    }
                }
            }
        }
    }
#pragma unroll
    for (int mi = 0; mi < MT; mi++) {
        const int m = mbase + mi * 16 + li;
        if (m >= p.M) continue;
        const bool first_img = rv_two && (m / p.rows_per_batch == img0);
#pragma unroll
        for (int pr = 0; pr < PR; pr++) {
            const bool paired = (2 * pr + 1) < NT;
            const int cnt = paired ? 8 : 4;
            const int n = nbase + 32 * pr + lg * cnt;
            if (n >= p.N) continue;
            float v[8];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                v[r] = acc[2 * pr][mi][r];
                v[4 + r] = paired ? acc[(2 * pr + 1) < NT ? 2 * pr + 1 : 2 * pr][mi][r] : 0.f;
            }
#pragma unroll
            for (int e = 0; e < 8; e++) {
                float x = v[e] * p.alpha + pre.b[pr][e];
                if (rv_two) x += first_img ? rvv[0][pr][e >> 2][e & 3] : rvv[1][pr][e >> 2][e & 3];
                else if (GENERIC && has_rv) x += p.rowvec[(size_t)(m / p.rows_per_batch) * p.ldrv + n + e];
                if (has_res) x += bf2f(rsv[mi][pr][e]);
                if (GENERIC && (flags & F_SILU)) x = silu_f(x);
                v[e] = x;
            }
#ifdef SIDLSG_EXP_NOSTORE      // measurement build: everything but the global stores
            if (v[0] != 123456.75f) continue;
#endif
            if (GENERIC && (flags & F_OUT_F32)) {
                float* c = reinterpret_cast<float*>(p.C) + (size_t)m * p.ldc + n;
                if (flags & F_ACCUM) {
                    for (int e = 0; e < cnt; e++) c[e] += v[e];
                } else {
                    *reinterpret_cast<f32x4*>(c) = (f32x4){v[0], v[1], v[2], v[3]};
                    if (cnt == 8) *reinterpret_cast<f32x4*>(c + 4) = (f32x4){v[4], v[5], v[6], v[7]};
                }
            } else {
                bf16* c = stage ? stage + (m - tm0) * ldr + (n - tn0) : reinterpret_cast<bf16*>(p.C) + (size_t)m * p.ldc + n;
                if (cnt == 8) {
                    bf16x8 o;
#pragma unroll
                    for (int e = 0; e < 8; e++) o[e] = f2bf(v[e]);
                    st8(c, o);
                } else {
                    bf16x4 o;
#pragma unroll
                    for (int e = 0; e < 4; e++) o[e] = f2bf(v[e]);
                    *reinterpret_cast<bf16x4*>(c) = o;
                }
            }
        }
    }
}

template <int MT, int NT, bool HOT = true>       // HOT = false: the caller has already peeled the hot combinations off
DEVFN void gemm_epilogue(const GemmParams& p, f32x4 (&acc)[NT][MT], int mbase, int nbase, int li, int lg,
                         const EpiPre<NT>& pre, bf16* stage = nullptr, int tm0 = 0, int tn0 = 0, int ldr = 0) {
    constexpr int PR = (NT + 1) / 2;
    if ((p.N & 7) == 0) {
        // ---- N % 8 == 0: every lane's 8 (4) channels are all in range or all out of range
        const bool plain = HOT && !(p.flags & (F_SILU | F_OUT_F32 | F_ACCUM));
#ifndef SIDLSG_EXP_GENERIC_EPILOGUE
        if (plain && !p.rowvec) {
            if (!p.res) epilogue_rows8<MT, NT, 0>(p, acc, mbase, nbase, li, lg, pre, stage, tm0, tn0, ldr);
            else epilogue_rows8<MT, NT, 1>(p, acc, mbase, nbase, li, lg, pre, stage, tm0, tn0, ldr);
        } else if (plain && !p.res && p.rows_per_batch >= 16 * MT) {
            epilogue_rows8<MT, NT, 2>(p, acc, mbase, nbase, li, lg, pre, stage, tm0, tn0, ldr);
        } else
#endif
        {
            (void)plain;
            epilogue_rows8<MT, NT, 4>(p, acc, mbase, nbase, li, lg, pre, stage, tm0, tn0, ldr);
        }
        return;
    }
    // ---- ragged N: element-wise, guarded
#pragma unroll
    for (int mi = 0; mi < MT; mi++) {
        const int m = mbase + mi * 16 + li;
        if (m >= p.M) continue;
        const float* rv = p.rowvec ? p.rowvec + (size_t)(m / p.rows_per_batch) * p.ldrv : nullptr;
#pragma unroll
        for (int pr = 0; pr < PR; pr++) {
            const bool paired = (2 * pr + 1) < NT;
            const int cnt = paired ? 8 : 4;
            const int n = nbase + 32 * pr + lg * cnt;
            float v[8];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                v[r] = acc[2 * pr][mi][r];
                v[4 + r] = paired ? acc[(2 * pr + 1) < NT ? 2 * pr + 1 : 2 * pr][mi][r] : 0.f;
            }
            for (int e = 0; e < cnt; e++) {
                const int nn = n + e;
                if (nn >= p.N) break;
                float x = v[e] * p.alpha;
                if (p.bias) x += p.bias[nn];
                if (rv) x += rv[nn];
                if (p.res) x += bf2f(p.res[(size_t)m * p.ldres + nn]);
                if (p.flags & F_SILU) x = silu_f(x);
                if (p.flags & F_OUT_F32) {
                    float* c = reinterpret_cast<float*>(p.C) + (size_t)m * p.ldc + nn;
                    *c = (p.flags & F_ACCUM) ? *c + x : x;
                } else {
                    reinterpret_cast<bf16*>(p.C)[(size_t)m * p.ldc + nn] = f2bf(x);
                }
            }
        }
    }
}

// Output row m of a 3x3 conv as a row of the implicit GEMM: its image b and output pixel (ho, wo), and from those the top-left input
// coordinate of its window, (ho * stride - pad, wo * stride - pad); a row m >= M gets hi = -100000, which pushes every tap out of range.
// (hi / wi are evaluated where the caller names them: the kernels' instruction order, and with it their code, stays what it was.)
struct ConvRow {
    int b, ho, wo;
    bool ok;
    DEVFN int hi(const GemmParams& p, int pad) const { return ok ? ho * p.stride - pad : -100000; }
    DEVFN int wi(const GemmParams& p, int pad) const { return wo * p.stride - pad; }
};
DEVFN ConvRow conv_row(const GemmParams& p, int m) {
    const bool ok = m < p.M;
    const int mm = ok ? m : 0;
    const int hw = p.Ho * p.Wo;
    const int b = mm / hw, rem = mm - b * hw;
    const int ho = rem / p.Wo, wo = rem - ho * p.Wo;
    return {b, ho, wo, ok};
}

// Row-major write-out of a BM x BN bf16 output tile staged in LDS by gemm_epilogue(stage=...).  In the MFMA accumulator
// layout one store instruction covers 16 rows x 64 bytes: half cache lines, which the L2 takes at half its write rate
// (FF-in 65536 x 2560 x 320: 335 MB of output left at 2.2 TB/s and were 58 % of the kernel -- the one-K-tile build of
// tools/ab/ffin.py).  From LDS, consecutive lanes write consecutive 16-byte chunks of a row: BN*2-byte contiguous runs.
template <int BM, int BN>
DEVFN void gemm_store_rows(const GemmParams& p, const bf16* stage, int m0, int n0, int ldr, int tid) {
    constexpr int CPR = BN / 8;                 // 16-byte chunks per row
#pragma unroll
    for (int i = 0; i < (BM * CPR + NTHREADS - 1) / NTHREADS; i++) {
        const int c = tid + i * NTHREADS;
        const int row = c / CPR, col = (c - row * CPR) * 8;
        if ((BM * CPR) % NTHREADS != 0 && row >= BM) break;
        const int m = m0 + row, n = n0 + col;
        if (m < p.M && n < p.N) st8(reinterpret_cast<bf16*>(p.C) + (size_t)m * p.ldc + n, *reinterpret_cast<const bf16x8*>(stage + row * ldr + col));
    }
}

// ---------------------------------------------------------------------------------------------
// Direct-to-LDS (buffer_load ... lds) kernels.  (A 256 x 160 / 8-wave / 3-stage-ring variant "v2" and a
// 256 x 160 / one-wave-per-SIMD / 32x32x16-MFMA variant "v5" were built and measured -- both correct, both slower
// than v3 on every SD shape; they live in the git history, not in the build.)
typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

// buffer_load_dwordx4 ... lds as inline assembly (64 lanes x 16 bytes -> LDS at `dst` + 16 * lane; dst wave-uniform).
// Measurement switch (-DSIDLSG_WGRAD_ASM_DMA=1), off in the build.  Background: the compiler's waitcnt pass tracks every
// LDS-DMA issued through __builtin_amdgcn_raw_ptr_buffer_load_lds and puts s_waitcnt vmcnt(0) in front of the next
// ds_read_b64_tr_b16 (always) or aliasing plain LDS read -- in the weight-gradient kernel that is the kk=1 fragment reads of
// the NEXT stage, half a stage after the DMA was issued, so the prefetch distance is half of what the schedule intends (seen
// in the ISA).  With the DMA invisible to the compiler the only wait is the explicit one at the publish barrier: measured
// +2-4 % on the dense weight gradients, -1-2 % on the conv ones (the asm statements pin the address arithmetic between them)
// -- like the early-DMA experiment in gemm_v3_kernel, more prefetch distance buys nothing.  (M0 is reserved: the compiler
// keeps nothing live in it.)
DEVFN void dma16_asm(__amdgpu_buffer_rsrc_t rs, const void* dst, unsigned voff, unsigned soff) {
    const unsigned la = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(lptr_t)dst);
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds" ::"s"(la), "v"(voff), "s"(rs), "s"(soff) : "memory");
}
#ifndef SIDLSG_MX8_SPREAD_DMA
#define SIDLSG_MX8_SPREAD_DMA 1
#endif
#ifndef SIDLSG_WGRAD_ASM_DMA
#define SIDLSG_WGRAD_ASM_DMA 0
#endif

// W-tile LDS swizzle (16-byte chunk index ^= wsw(row)).  A ds_read_b128 is serviced in the lane groups
// {0-3,12-15,20-27}, {4-11,16-19,28-31}, ... (MI355X guide, LDS table), and the W fragment rows of a paired (ni, ni+1)
// column block are li -> 8*(li>>2) + (li&3): with the plain (row>>1)&7 swizzle the lg=0 and lg=1 lanes of one group
// collide 2-way (measured: SQ_LDS_BANK_CONFLICT = 31 % of SQ_LDS_IDX_ACTIVE).  For those rows use
// (q&1) | ((q>>2)&3)<<1 with q = row>>1, which makes the 16 lanes of every group hit 16 distinct 16-byte slots; the
// trailing unpaired 16-row block (rows 64..79 of each wave's 80) keeps the plain swizzle.
DEVFN int wsw(int r) {
    const int rr = r >= 80 ? r - 80 : r;
    const int q = r >> 1;
    return rr < 64 ? ((q & 1) | (((q >> 2) & 3) << 1)) : (q & 7);
}

#ifdef SIDLSG_EXP_TRACE           // measurement build (tools/ab/gemm_trace.py): per-block phase timestamps, 100 MHz wall clock
static __device__ unsigned long long* g_trace = nullptr;      // one per unit: sidlsg_exp_set_trace (gemm.hip) sets its own and wgrad.hip's
static inline int exp_set_trace_here(void* ptr) { return hipMemcpyToSymbol(HIP_SYMBOL(g_trace), &ptr, sizeof(ptr)) == hipSuccess ? 0 : -1; }
int sidlsg_exp_set_trace_wgrad(void* ptr);
#define TRACE(i) do { if (g_trace && threadIdx.x == 0) g_trace[(size_t)blockIdx.x * 8 + (i)] = wall_clock64(); } while (0)
#define TRACE_HWID() do { if (g_trace && threadIdx.x == 0) { unsigned h, x; asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(h)); asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(x)); g_trace[(size_t)blockIdx.x * 8 + 7] = ((unsigned long long)x << 32) | h; } } while (0)
#define WTRACE(i) do { if (g_trace && threadIdx.x == 0) g_trace[(size_t)blockIdx.x * 8 + (i)] = wall_clock64(); } while (0)
#else
#define TRACE(i)
#define TRACE_HWID()
#define WTRACE(i)
#endif
#ifndef SIDLSG_CONV_TAP_INNER
#define SIDLSG_CONV_TAP_INNER 1
#endif
#ifndef SIDLSG_V3_SCHED_FENCE
#define SIDLSG_V3_SCHED_FENCE 1
#endif
#ifndef SIDLSG_V3_PRIO_PIN
#define SIDLSG_V3_PRIO_PIN 1   // 1: sched_barriers pin the MFMAs and scalar instructions relative to the flip (VALU / VMEM / LDS may cross)
#endif
#define V3_SETPRIO(v) do { if (SIDLSG_V3_PRIO_PIN) __builtin_amdgcn_sched_barrier(0x3F2); __builtin_amdgcn_s_setprio(v); if (SIDLSG_V3_PRIO_PIN) __builtin_amdgcn_sched_barrier(0x3F2); } while (0)
#ifndef SIDLSG_V3_PRIO
#define SIDLSG_V3_PRIO 0      // A/B knob (bit mask): s_setprio(1) around the MFMA clusters of a K-tile -- 1: gemm_v3 (dense / conv fwd + dgrad), 2: wgrad_v2 (two co-resident blocks per CU in different phases)
#endif

// ---- library state the contraction units reach (state.hip; sidlsg_det and sidlsg_ws_for_stream: common.h)
struct Ws { float* ptr; long long bytes; };
Ws ws_for(hipStream_t s);      // the split-K / pixel-split scratch of stream `s`; ptr null when none
int p8_mode();                 // -1 by rule, 0 never, 1 / 2 forced (SIDLSG_GEMM_P8, sidlsg_debug_set_p8)
int splitk_splits(long long tiles, int nk, long long mn, const Ws& w, int min_nk, int min_kt);
int splitk_splits_bf16(long long tiles, int nk, long long mn, const Ws& w);
// Second launch of a split-K GEMM: the `splits` slabs of p.ws -> C through the epilogue (gemm_finish_kernel and its launcher: gemm.hip)
void launch_gemm_finish(const GemmParams& p, int splits, hipStream_t s);

// Dispatch record (include/sidlsg_hip.h sidlsg_debug_last_launch): every host launcher of the three units and of gemm_p8.h says which kernel
// it is about to launch, just before its SIDLSG_LAUNCH -- plain stores to a thread-local struct, so the record is complete also when the launch
// fails.  A launcher of a second kernel (gemm_finish_kernel, the slab reductions) adds its bit to `finish`.
struct LaunchRecord { int v[SIDLSG_REC_INTS]; };
extern thread_local LaunchRecord g_last_launch;      // (state.hip)
static inline void record_launch(int kernel, int bm, int bn, int mode, int pad, int p8, int splits, int partial) {
    int* r = g_last_launch.v;
    r[SIDLSG_REC_KERNEL] = kernel; r[SIDLSG_REC_BM] = bm; r[SIDLSG_REC_BN] = bn; r[SIDLSG_REC_MODE] = mode; r[SIDLSG_REC_PAD] = pad;
    r[SIDLSG_REC_P8] = p8; r[SIDLSG_REC_SPLITS] = splits; r[SIDLSG_REC_PARTIAL] = partial; r[SIDLSG_REC_FINISH] = 0; r[SIDLSG_REC_SEQ]++;
}
static inline void record_followup(int fin) { g_last_launch.v[SIDLSG_REC_FINISH] |= fin; }
// a split-K GEMM launcher: `splits` slabs when p.kt_per_split is set
static inline int record_partial(int splits) { return splits > 1 ? SIDLSG_PART_SLABS : SIDLSG_PART_ONE; }

static int check_common(const GemmParams& p) {
    if (p.M <= 0 || p.N <= 0 || p.K <= 0) return SIDLSG_EINVAL;
    if ((p.K & 7) || (p.lda & 7)) return SIDLSG_EINVAL;            // 16-byte chunks
    if (!p.A || !p.W || !p.C) return SIDLSG_EINVAL;
    if (p.rowvec && p.rows_per_batch <= 0) return SIDLSG_EINVAL;
    if ((p.flags & F_ACCUM) && !(p.flags & F_OUT_F32)) return SIDLSG_EINVAL;
    return SIDLSG_OK;
}

// Operand contract of the output and the epilogue operands (include/sidlsg_hip.h "operand contract"): rows no narrower than the N columns
// the kernel touches, and -- N % 8 == 0: the vector epilogue (epilogue_rows8, gemm_store_rows, the p8 row-major epilogue, gemm_finish_kernel)
// moves 16 bytes per access at column offsets that are multiples of 8 (4 for fp32 data) -- strides and base addresses that keep those aligned.
static int check_epilogue(const GemmParams& p) {
    if (p.lda < (p.Cin ? p.Cin : p.K) || p.ldc < p.N || (p.res && p.ldres < p.N) || (p.rowvec && p.ldrv < p.N)) return SIDLSG_EINVAL;
    if ((p.N & 7) == 0) {
        auto misaligned = [](const void* q) { return ((uintptr_t)q & 15) != 0; };
        if ((p.ldc & ((p.flags & F_OUT_F32) ? 3 : 7)) || misaligned(p.C)) return SIDLSG_EINVAL;
        if (p.res && ((p.ldres & 7) || misaligned(p.res))) return SIDLSG_EINVAL;
        if (p.rowvec && ((p.ldrv & 3) || misaligned(p.rowvec))) return SIDLSG_EINVAL;
        if (misaligned(p.bias) || misaligned(p.bias1)) return SIDLSG_EINVAL;
    }
    return SIDLSG_OK;
}

// ---- host side of the entry points: filling GemmParams, operand ranges, the second set of a grouped call
static bool fits31(unsigned long long bytes) { return bytes < 0x7FFFFFFFull; }

// Byte range of an operand for its 31-bit buffer descriptor: `rows` rows of `ld` elements of `esize` bytes, `cols` of them used (a weight
// matrix: N rows with ld = cols = K, or 9 Cout rows of Cin; e4m3 operands: esize 1).  The check counts `halo` more elements, which `range` does not include.  False: the operand is too large.
static bool range31(unsigned& range, unsigned long long rows, int ld, int cols, int esize, unsigned long long halo = 0) {
    const unsigned long long bytes = ((rows - 1) * ld + cols) * esize;
    if (!fits31(bytes + halo * esize)) return false;
    range = (unsigned)bytes;
    return true;
}
// pixels of the image a 3x3 conv reads: `ups` reads a half-size source through a nearest x2 upsample
static unsigned long long conv_src_pixels(int B, int H, int Wd, int ups) { return (unsigned long long)B * (ups ? H / 2 : H) * (ups ? Wd / 2 : Wd); }

// Operands, epilogue and shape of a dense contraction.  The caller adds what its format needs (wscale, the GEGLU fields, the second set).
static GemmParams dense_params(const void* A, int lda, const void* W, void* C, int ldc, const float* bias, const void* res, int ldres,
                               const float* rowvec, int ld_rowvec, int rows_per_batch, int M, int N, int K, float alpha, int flags) {
    GemmParams p{};
    p.A = (const bf16*)A; p.W = (const bf16*)W; p.C = C; p.bias = bias; p.res = (const bf16*)res; p.rowvec = rowvec;
    p.ldrv = ld_rowvec > 0 ? ld_rowvec : N;
    p.M = M; p.N = N; p.K = K; p.lda = lda; p.ldc = ldc; p.ldres = ldres; p.rows_per_batch = rows_per_batch;
    p.alpha = alpha; p.flags = flags;
    return p;
}
// The same for a 3x3 conv (pad 1) as an implicit GEMM: M = output pixels, K = 9 taps x Cin, one row-vector row per image.  stride: 1 or 2.
static GemmParams conv_params(const void* X, int ldx, const void* W, void* Y, int ldc, const float* bias, const void* res, int ldres,
                              const float* rowvec, int ld_rowvec, int B, int H, int Wd, int Cin, int Cout, int stride, int ups, float alpha,
                              int flags) {
    const int Ho = (H + 2 - 3) / stride + 1, Wo = (Wd + 2 - 3) / stride + 1;
    GemmParams p = dense_params(X, ldx, W, Y, ldc, bias, res, ldres, rowvec, ld_rowvec, Ho * Wo, B * Ho * Wo, Cout, 9 * Cin, alpha, flags);
    p.H = H; p.Wd = Wd; p.Cin = Cin; p.stride = stride; p.ups = ups; p.Ho = Ho; p.Wo = Wo;
    return p;
}

// The grouped forms (sidlsg_*_g2, include/sidlsg_hip.h "grouped launches"): a second set (W1, wscale1, bias1) for the rows / samples of the
// second half; g2 = false: the ordinary launch (Mg = 0), exactly as before the grouped forms existed.  bf16 weights have no wscale1; the
// e4m3 entry points check theirs.
static void set_group2(GemmParams& p, bool g2, const void* W1, const float* wscale1, const float* bias1) {
    if (!g2) return;
    p.W1 = (const bf16*)W1; p.wscale1 = wscale1; p.bias1 = bias1; p.Mg = p.M / 2;
}
static bool group2_args_ok(int rows, const void* W1, const float* bias, const float* bias1) {
    return W1 && !(rows & 1) && (bias != nullptr) == (bias1 != nullptr);
}
