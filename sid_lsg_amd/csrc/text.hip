// CLIP text encoder (gfx950): causal self-attention for short sequences and the token + position embedding.
//
// sidlsg_attn_causal_fwd(_f32): O = softmax(mask(Q K^T D^-1/2)) V per head, key j visible to query i iff j <= i, 1 <= N <= 128
// (CLIP: 77), D a multiple of 8 up to 128 (tiled at DP = D rounded up to 32 for bf16, to 16 for fp32; the pad columns of Q, K and V
// are zeros).  Forward only, no LSE: the text encoder is frozen.  A composition of the short-key core of attn_short.h (staging,
// Q operands, scores, single-pass softmax, PV, store; the bf16 fragment helpers come from attn_frag.h):
//   - one workgroup per (batch, head); wave w owns queries 16 w .. 16 w + 15, so a block is ceil(N / 16) waves (1 .. 8);
//   - the head's whole K and V are staged in LDS once (rows past N as zeros) and published by ONE barrier: bf16 rows padded to
//     tile_ld() (an odd multiple of 32 bytes), 2 * 128 * 144 * 2 = 72 KB at N = D = 128, 30 KB for CLIP-L (N = 77 -> 96 rows of 80);
//     fp32 rows padded to DP + 4, 2 * 80 * 68 * 4 = 43 KB for CLIP-L, 132 KB at the maximum;
//   - wave w visits the 16-key sub-tiles 0 .. w only: the causal half is skipped, not computed and masked.  Only the diagonal
//     sub-tile (and key columns >= N) is masked to -inf, before the row maximum; key 0 is visible to every row, so the maximum is
//     finite and no NaN can arise;
//   - the softmax calls exp2f in both dtypes;
//   - query rows >= N are never stored.
//
// sidlsg_text_embed(_f32): out[b L + l][:] = tok[ids[b][l]][:] + pos[l][:], summed in fp32 and rounded once at the store.  An id
// outside [0, V) reads nothing and writes its row as NaN.
#include "attn_short.h"

namespace {

constexpr int CMAXN = SHORT_MAXN;  // longest sequence: 8 waves of 16 queries

template <typename T>
struct CausalParams {
    const T *Q, *K, *V;
    T* O;
    int H, N, D;                   // D <= DP, the width the kernel is tiled for: columns D .. DP - 1 are staged / loaded as zeros
    int ldq, ldk, ldv, ldo;
    long long bsq, bsk, bsv, bso;
    float scale2;                  // D^-0.5 * log2(e)
};

template <typename T, int DP>
__global__ __launch_bounds__(512) void attn_causal_kernel(CausalParams<T> p) {
    constexpr int LD = short_ld<T, DP>(), DT = DP / 16;
    extern __shared__ __attribute__((aligned(16))) char smem_c[];
    const int N = p.N, D = p.D;
    const int NR = short_rows<T>(N);
    T* Ks = reinterpret_cast<T*>(smem_c);            // [NR][LD]
    T* Vs = Ks + NR * LD;                            // [NR][LD]
    const int b = blockIdx.x / p.H, h = blockIdx.x % p.H;
    const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, lg = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);      // in an SGPR: the sub-tile tests of the core are scalar branches
    short_stage<T, DP>(Ks, Vs, p.K + b * p.bsk + h * D, p.V + b * p.bsv + h * D, p.ldk, p.ldv, NR, N, D, tid, blockDim.x);
    const int q = 16 * w + li;                       // rows >= N of the last wave take part with row 0's operands
    ShortQ<T, DP> qf;
    qf.load(p.Q + b * p.bsq + h * D, q, N, p.ldq, D, lg);
    __syncthreads();

    f32x4 sc[SHORT_MAXSUB], acc[DT];
    short_scores<T, DP, SHORT_MAXSUB, true>(sc, Ks, qf, w + 1, N, p.scale2, q, li, lg);      // sub-tiles 0 .. w
    const float l = short_softmax<SHORT_MAXSUB, false>(sc);
#pragma unroll
    for (int i = 0; i < DT; i++) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    short_pv<T, DP, SHORT_MAXSUB>(acc, Vs, sc, w + 1, li, lg);
    if (q >= N) return;
    short_store<T, DP>(p.O + b * p.bso + h * D + (long long)q * p.ldo, acc, 1.0f / l, D, lg);
}

template <typename T, int DP>
size_t causal_lds_bytes(int N) { return short_lds_bytes<T, DP>(short_rows<T>(N)); }

template <typename T, int DP>
int launch_causal(const CausalParams<T>& p, int B, hipStream_t s) {
    if (const int e = sidlsg_lds_limit<&attn_causal_kernel<T, DP>>(causal_lds_bytes<T, DP>(CMAXN))) return e;
    const dim3 grid((unsigned)(B * p.H)), block((unsigned)(64 * ((p.N + 15) / 16)));
    SidlsgTraceScope ts(SIDLSG_FAM_ATTN_FWD, 2.0 * B * p.H * (double)p.N * p.N * p.D, 4.0 * sizeof(T) * B * p.H * (double)p.N * p.D);
    const size_t lds = causal_lds_bytes<T, DP>(p.N);
    SIDLSG_LAUNCH((attn_causal_kernel<T, DP>), grid, block, lds, s, p);
    return sidlsg_last_error();
}

template <typename T>
int attn_causal_t(const void* Q, const void* K, const void* V, void* O, int B, int H, int N, int D, int ldq, int ldk, int ldv, int ldo,
                  long long bsq, long long bsk, long long bsv, long long bso, void* stream) {
    if (B <= 0 || H <= 0 || N < 1 || N > CMAXN) return SIDLSG_EINVAL;
    if (D < 8 || D > 128 || (D & 7)) return SIDLSG_EINVAL;
    if ((long long)B * H >= (1LL << 31)) return SIDLSG_EINVAL;
    if (!attn_views_ok<T>({{Q, ldq, bsq}, {K, ldk, bsk}, {V, ldv, bsv}, {O, ldo, bso}}, (long long)H * D)) return SIDLSG_EINVAL;
    CausalParams<T> p;
    p.Q = (const T*)Q; p.K = (const T*)K; p.V = (const T*)V; p.O = (T*)O;
    p.H = H; p.N = N; p.D = D; p.ldq = ldq; p.ldk = ldk; p.ldv = ldv; p.ldo = ldo; p.bsq = bsq; p.bsk = bsk; p.bsv = bsv; p.bso = bso;
    p.scale2 = (float)(1.4426950408889634 / sqrt((double)D));
    return attn_width_dispatch<short_tile<T>(), 128>(D, [&](auto dp) { return launch_causal<T, decltype(dp)::value>(p, B, (hipStream_t)stream); });
}

template <typename T>
__global__ __launch_bounds__(256) void text_embed_kernel(const long long* __restrict__ ids, const float* __restrict__ tok,
                                                         const float* __restrict__ pos, T* __restrict__ out, int rows, int L, int D, int V) {
    const int nch = D >> 3;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)rows * nch) return;
    const int row = (int)(idx / nch), c = (int)(idx % nch) * 8;
    const long long id = ids[row];
    float v[8];
    if (id < 0 || id >= V) {                         // nothing is read for an id outside the table; the row is loud instead
#pragma unroll
        for (int e = 0; e < 8; e++) v[e] = __builtin_nanf("");
    } else {
        float t[8], q[8];
        ldv8<float>(tok + id * D + c, t);
        ldv8<float>(pos + (long long)(row % L) * D + c, q);
#pragma unroll
        for (int e = 0; e < 8; e++) v[e] = t[e] + q[e];
    }
    stv8<T>(out + (long long)row * D + c, v);
}

template <typename T>
int text_embed_t(const void* ids, const float* tok, const float* pos, void* out, int B, int L, int D, int V, int P, void* stream) {
    if (!ids || !tok || !pos || !out || B <= 0 || L <= 0 || D <= 0 || V <= 0 || P <= 0 || L > P || (D & 7)) return SIDLSG_EINVAL;
    if (((uintptr_t)tok | (uintptr_t)pos | (uintptr_t)out) & 15 || ((uintptr_t)ids & 7)) return SIDLSG_EINVAL;
    const long long rows = (long long)B * L, n = rows * (D >> 3);
    if (rows * D >= (1LL << 31)) return SIDLSG_EINVAL;
    hipLaunchKernelGGL(text_embed_kernel<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const long long*)ids, tok,
                       pos, (T*)out, (int)rows, L, D, V);
    return sidlsg_last_error();
}

}  // namespace

extern "C" {

int sidlsg_attn_causal_fwd(const void* Q, const void* K, const void* V, void* O, int B, int H, int N, int D, int ldq, int ldk, int ldv,
                           int ldo, long long bsq, long long bsk, long long bsv, long long bso, void* stream) {
    return attn_causal_t<bf16>(Q, K, V, O, B, H, N, D, ldq, ldk, ldv, ldo, bsq, bsk, bsv, bso, stream);
}
int sidlsg_attn_causal_fwd_f32(const void* Q, const void* K, const void* V, void* O, int B, int H, int N, int D, int ldq, int ldk, int ldv,
                               int ldo, long long bsq, long long bsk, long long bsv, long long bso, void* stream) {
    return attn_causal_t<float>(Q, K, V, O, B, H, N, D, ldq, ldk, ldv, ldo, bsq, bsk, bsv, bso, stream);
}

int sidlsg_text_embed(const void* ids, const float* tok, const float* pos, void* out, int B, int L, int D, int V, int P, void* stream) {
    return text_embed_t<bf16>(ids, tok, pos, out, B, L, D, V, P, stream);
}
int sidlsg_text_embed_f32(const void* ids, const float* tok, const float* pos, void* out, int B, int L, int D, int V, int P, void* stream) {
    return text_embed_t<float>(ids, tok, pos, out, B, L, D, V, P, stream);
}

}  // extern "C"
