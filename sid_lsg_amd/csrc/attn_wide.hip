// Forward-only flash attention for ONE wide head, D = 512 (gfx950): the mid-block attention of the Stable Diffusion VAE
// (diffusers AutoencoderKL: Attention(heads = 1, dim_head = 512) over (H/8)*(W/8) tokens -- 4096 at 512^2, 9216 at 768^2).
// The kernels of attention.hip stop at D <= 160: their tiles, register budget and occupancy are built around d = 40 .. 160.
//
// Same orientation trick as attention.hip (no LDS round trip for P): S^T[key][query] = mfma(A = K rows, B = Q rows), whose
// accumulator layout (lane: column = query, 4 consecutive keys) is the B operand of O^T[d][query] += mfma(A = V^T, B = P^T) with V^T
// taken from the row-major V tile by ds_read_b64_tr_b16.  Softmax statistics are per query = per lane, replicated over the 4 lane groups.
//
// Sizing, from D = 512 (not from the d = 40 kernels):
//   - a wave owns 16 queries: O^T is 32 d-tiles x f32x4 = 128 accumulator registers per lane; its Q rows as MFMA operands are
//     16 k-slices x bf16x8 = 64 registers; a K + V tile in flight global -> registers -> LDS is another 64.  ~290 registers with the
//     rest: one wave per SIMD (512-register file), so a block is 4 waves = 64 queries and __launch_bounds__(256, 1).
//   - a 32-key tile of K and of V is 2 x 32 KB of bf16; rows are padded to 528 elements (an odd multiple of 32 bytes: conflict-free
//     for the ds_read_b128 row reads and the transposed reads alike, see tile_ld() of attn_frag.h) -> 66 KB per stage, double
//     buffered = 132 KB of the CU's 160 KB.  With one wave per SIMD nothing else hides HBM / L2 latency, so the next tile's loads
//     are issued before the current tile's MFMAs and committed to the other buffer after them: one barrier per key tile.
//   - per tile and wave: 32 MFMAs for S^T (2 key sub-tiles x 16 k-slices), 32 for O^T (32 d-tiles); 32 ds_read_b128 + 64 transposed reads.
// The O^T rescale (128 multiplies per lane) runs only on tiles where some query of the wave saw its running maximum grow (exactly: no
// deferral threshold), which is the common case only in the first few tiles.
// The row stride (tile_ld), the transposed read of V (tr_frag32) and pack_p are the shared ones of attn_frag.h.
// N (queries = keys) is a multiple of 16; a trailing half tile of keys is masked to -inf, rows past N of the last block are idle waves.
#include "attn_frag.h"
#include <math.h>

namespace {

constexpr int WD = 512;            // head width
constexpr int WLD = tile_ld<WD>();  // LDS row stride (elements): 528
constexpr int WKT = 32;            // keys per tile
constexpr int WNS = WD / 32;       // k-slices of the QK^T contraction
constexpr int WDT = WD / 16;       // output d-tiles
constexpr int WTILE = WKT * WLD;   // elements of one staged tile
constexpr int WPER = WKT * (WD / 8) / 256;   // 16-byte chunks per thread per tile (8)

struct WideParams {
    const bf16 *Q, *K, *V;
    bf16* O;
    int N;
    int ldq, ldk, ldv, ldo;
    long long bsq, bsk, bsv, bso;
    float scale2;                  // D^-0.5 * log2(e)
};

__global__ __launch_bounds__(256, 1) void attn_wide_kernel(WideParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem_w[];
    bf16* Ks = reinterpret_cast<bf16*>(smem_w);      // [2][WTILE]
    bf16* Vs = Ks + 2 * WTILE;                       // [2][WTILE]
    const int b = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lg = lane >> 4;
    const int q0 = (blockIdx.x * 4 + wave) * 16;
    const bool active = q0 < p.N;                    // wave-uniform (N % 16 == 0)
    const long long kbytes = ((long long)(p.N - 1) * p.ldk + WD) * 2, vbytes = ((long long)(p.N - 1) * p.ldv + WD) * 2;
    const __amdgpu_buffer_rsrc_t rk = mk_buf(p.K + b * p.bsk, kbytes);      // rows >= N read zeros
    const __amdgpu_buffer_rsrc_t rv = mk_buf(p.V + b * p.bsv, vbytes);

    // staging map: chunk idx = tid + 256 j -> tile row (tid >> 6) + 4 j, columns 8 (tid & 63) ..: a wave moves one whole row per j
    const int srow = tid >> 6, scol = (tid & 63) * 8;
    bf16x8 kreg[WPER], vreg[WPER];
    auto load_tile = [&](int k0) {
#pragma unroll
        for (int j = 0; j < WPER; j++) {
            const unsigned r = (unsigned)(k0 + srow + 4 * j);
            kreg[j] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rk, (r * (unsigned)p.ldk + scol) * 2u, 0, 0));
            vreg[j] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rv, (r * (unsigned)p.ldv + scol) * 2u, 0, 0));
        }
    };
    auto store_tile = [&](int buf) {
#pragma unroll
        for (int j = 0; j < WPER; j++) {
            st8(Ks + buf * WTILE + (srow + 4 * j) * WLD + scol, kreg[j]);
            st8(Vs + buf * WTILE + (srow + 4 * j) * WLD + scol, vreg[j]);
        }
    };

    // Q rows as B operands: lane (li, lg) holds Q[q0 + li][32 s + 8 lg .. + 8]
    bf16x8 qf[WNS];
    {
        const bf16* qrow = p.Q + b * p.bsq + (long long)(active ? q0 + li : 0) * p.ldq + lg * 8;
#pragma unroll
        for (int s = 0; s < WNS; s++) qf[s] = ld8(qrow + s * 32);
    }
    f32x4 acc[WDT];
#pragma unroll
    for (int i = 0; i < WDT; i++) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, l = 0.f;        // running maximum (log2 units) and this lane group's share of the denominator

    const int ntiles = (p.N + WKT - 1) / WKT;
    load_tile(0);
    store_tile(0);
    __syncthreads();
    for (int t = 0; t < ntiles; t++) {
        const int buf = t & 1;
        if (t + 1 < ntiles) load_tile((t + 1) * WKT);
        if (active) {
            const bf16* kt = Ks + buf * WTILE;
            const bf16* vt = Vs + buf * WTILE;
            f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < WNS; s++) {
                const bf16x8 ka = *reinterpret_cast<const bf16x8*>(kt + li * WLD + s * 32 + lg * 8);
                const bf16x8 kb = *reinterpret_cast<const bf16x8*>(kt + (16 + li) * WLD + s * 32 + lg * 8);
                s0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ka, qf[s], s0, 0, 0, 0);
                s1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kb, qf[s], s1, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; r++) { s0[r] *= p.scale2; s1[r] *= p.scale2; }
            if (t * WKT + 16 >= p.N) {               // the trailing half tile: keys 16 .. 31 of it do not exist (wave-uniform)
#pragma unroll
                for (int r = 0; r < 4; r++) s1[r] = -INFINITY;
            }
            float mx = fmaxf(fmaxf(fmaxf(s0[0], s0[1]), fmaxf(s0[2], s0[3])), fmaxf(fmaxf(s1[0], s1[1]), fmaxf(s1[2], s1[3])));
            mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            const float mn = fmaxf(m, mx);
            if (__any(mn > m)) {                     // some query's maximum grew: everything accumulated at the old maximum is rescaled, once
                const float alpha = exp2f(m - mn);   // first tile: exp2(-inf) = 0 on zero accumulators
                l *= alpha;
#pragma unroll
                for (int i = 0; i < WDT; i++)
#pragma unroll
                    for (int r = 0; r < 4; r++) acc[i][r] *= alpha;
                m = mn;
            }
            float ps = 0.f;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                s0[r] = exp2f(s0[r] - m);
                s1[r] = exp2f(s1[r] - m);
                ps += s0[r] + s1[r];
            }
            l += ps;
            const bf16x8 pf = pack_p(s0, s1);
#pragma unroll
            for (int i = 0; i < WDT; i++) acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag32(vt, WLD, 0, i * 16, li, lg), pf, acc[i], 0, 0, 0);
        }
        if (t + 1 < ntiles) store_tile(buf ^ 1);     // that buffer was last read in iteration t - 1, before its closing barrier
        __syncthreads();
    }
    if (!active) return;
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    const float inv = 1.0f / l;
    bf16* orow = p.O + b * p.bso + (long long)(q0 + li) * p.ldo + lg * 4;    // lane: query li, channels 16 i + 4 lg .. + 4
#pragma unroll
    for (int i = 0; i < WDT; i++) {
        const bf16x4 o = {f2bf(acc[i][0] * inv), f2bf(acc[i][1] * inv), f2bf(acc[i][2] * inv), f2bf(acc[i][3] * inv)};
        *reinterpret_cast<bf16x4*>(orow + i * 16) = o;
    }
}

}  // namespace

extern "C" {

// O = softmax(Q K^T D^-1/2) V for one head of width D = 512; Q/K/V/O: [B][N][ld*] bf16 views (token stride ld*, batch stride bs*, in
// elements), N a multiple of 16.  Forward only, no LSE.
int sidlsg_attn_fwd_wide(const void* Q, const void* K, const void* V, void* O, int B, int N, int D, int ldq, int ldk, int ldv, int ldo,
                         long long bsq, long long bsk, long long bsv, long long bso, void* stream) {
    if (D != WD || !Q || !K || !V || !O || B <= 0 || B > 65535 || N <= 0 || (N & 15)) return SIDLSG_EINVAL;
    if (ldq < D || ldk < D || ldv < D || ldo < D || ((ldq | ldk | ldv | ldo) & 7) || ((bsq | bsk | bsv | bso) & 7)) return SIDLSG_EINVAL;
    if ((((uintptr_t)Q | (uintptr_t)K | (uintptr_t)V) & 15) || ((uintptr_t)O & 7)) return SIDLSG_EINVAL;
    // 32-bit byte offsets inside one batch (the staged tile may reach 31 rows past N: those offsets must not wrap either)
    const long long lim = 0x7FFFFFFFll;
    if (((long long)N + WKT) * ldk * 2 >= lim || ((long long)N + WKT) * ldv * 2 >= lim) return SIDLSG_EINVAL;
    WideParams p;
    p.Q = (const bf16*)Q; p.K = (const bf16*)K; p.V = (const bf16*)V; p.O = (bf16*)O;
    p.N = N; p.ldq = ldq; p.ldk = ldk; p.ldv = ldv; p.ldo = ldo; p.bsq = bsq; p.bsk = bsk; p.bsv = bsv; p.bso = bso;
    p.scale2 = (float)(1.4426950408889634 / sqrt((double)D));
    const size_t lds = (size_t)4 * WTILE * sizeof(bf16);
    if (const int e = sidlsg_lds_limit<&attn_wide_kernel>(lds)) return e;
    SidlsgTraceScope ts(SIDLSG_FAM_ATTN_FWD, 4.0 * B * (double)N * N * D, 8.0 * B * (double)N * D);
    SIDLSG_LAUNCH(attn_wide_kernel, dim3((unsigned)((N + 63) / 64), (unsigned)B), dim3(256), lds, (hipStream_t)stream, p);
    return sidlsg_last_error();
}

}  // extern "C"
