// Decoupled cross-attention of an image-prompt adapter (gfx950): two key sets, two softmaxes, ONE launch.
//
// sidlsg_attn_cross2_fwd(_ps, _f32):  O = softmax(Q K^T D^-1/2) V + s * softmax(Q K2^T D^-1/2) V2  per head.  The first set is the
// text (1 <= Nk <= 128 keys, 77 for SD), the second the image tokens (1 <= Nk2 <= 32, 4 for the published SD 1.5 adapters); any
// Nq >= 1.  bf16: D a multiple of 8 up to 160, tiled at DP = D rounded up to 32; fp32: D a multiple of 4 up to 160, tiled at
// DP = D rounded up to 16; the pad columns of Q, K and V are zeros.  Forward only, no LSE: the adapter runs in sampling passes.
// A composition of the short-key core of attn_short.h (staging, Q operands, scores, single-pass softmax, PV, store -- orientation,
// MFMA forms and LDS layout are described there; the bf16 fragment helpers come from attn_frag.h):
//   - a workgroup is 8 waves and owns `tpb` consecutive 16-query tiles of one (batch, head); wave w takes tiles w, w + 8, ...;
//   - both key sets of the (batch, head) are staged in LDS once per workgroup (rows past Nk / Nk2 as zeros) and published by ONE
//     barrier: bf16 (128 + 32) * 176 * 2 * 2 = 110 KB at the maximum, 41 KB for SD's 77 + 4 keys at D = 40 (96 + 32 rows of 80),
//     90 KB at D = 160.  K / V are re-staged per workgroup and the staging is what a short launch waits for, so a workgroup is as
//     large as the hardware allows: tpb = 8 (128 queries, one tile per wave) below 2048 queries, 32 (512 queries) from there on.
//     Measured at SD 1.5's shapes (B 16, H 8, 77 + 4 keys; profiles/ip_adapter.txt): 4 waves with tpb 4 / 16 took 45 / 37 / 25 /
//     11 us at (Nq, D) = (4096, 40) / (1024, 80) / (256, 160) / (64, 160), 8 waves take 39 / 21 / 12 / 11 us;
//   - sub-tiles with 16 j >= Nk (>= Nk2) are skipped and key columns >= Nk (>= Nk2) are masked to -inf before the row maximum; key 0
//     of either set is never masked, so both maxima are finite.  At most (8 + 2) sub-tiles x 4 scores per lane live in registers;
//   - each set is normalised on its own, and both share ONE fp32 accumulator: acc = P2~ V2 (P~ = exp2(score - max), un-normalised, so
//     the largest probability of a row is exactly 1), acc *= s l / l2, acc += P~ V, O = acc / l -- the sum is rounded once, at the
//     store.  bf16: P~ is rounded to bf16 once in front of the PV contraction; fp32: nothing is rounded to bf16;
//   - the two dtypes differ in three more things, each a constant of Cross2Kind below: the exponential, the Q prefetch and the
//     staged size of the image set;
//   - s == 0 skips the image set altogether: K2 / V2 are not read, and the result is the one-set attention of this kernel;
//   - query rows >= Nq are never stored.
#include "attn_short.h"

namespace {

constexpr int X2_MAXN = SHORT_MAXN;    // text keys
constexpr int X2_MAXN2 = 32;           // image keys: one 32-key tile
constexpr int X2_SUB2 = X2_MAXN2 / 16;
constexpr int X2_WAVES = 8;
constexpr size_t X2_LDS_MAX = 160 * 1024;

template <typename T>
struct Cross2Params {
    const T *Q, *K, *V, *K2, *V2;
    T* O;
    int H, Nq, Nk, Nk2, D;         // D <= DP, the width the kernel is tiled for: columns D .. DP - 1 are staged / loaded as zeros
    int tpb, nchunk;               // 16-query tiles per workgroup; workgroups per (batch, head)
    int ldq, ldk, ldv, ldk2, ldv2, ldo;
    long long bsq, bsk, bsv, bsk2, bsv2, bso;
    float scale2;                  // D^-0.5 * log2(e); 1 for pre-scaled queries
    float s;
};

// What the bf16 and fp32 kernels do differently beyond the element-type rules of the core
template <typename T>
struct Cross2Kind {
    static constexpr bool HALF = sizeof(T) == 2;
    static constexpr bool FAST_EXP = HALF;       // bf16: v_exp_f32 directly (short_softmax); fp32: exp2f
    static constexpr bool Q_PREFETCH = HALF;     // bf16: the next tile's Q rows are requested before this tile's arithmetic, so a wave's
                                                 // tiles do not each expose a global-load latency; fp32: loaded at the top of the tile
    // staged image rows.  bf16: always the one 32-key tile (a compile-time loop bound); fp32: the whole 16-key sub-tiles of Nk2
    static constexpr int rows2(int Nk2) { return HALF ? X2_MAXN2 : short_rows<T>(Nk2); }
};

template <typename T, int DP>
__global__ __launch_bounds__(64 * X2_WAVES) void attn_cross2_kernel(Cross2Params<T> p) {
    typedef Cross2Kind<T> Kind;
    constexpr int LD = short_ld<T, DP>(), DT = DP / 16;
    extern __shared__ __attribute__((aligned(16))) char smem_x[];
    const int Nq = p.Nq, Nk = p.Nk, Nk2 = p.Nk2, D = p.D;
    const int NR = short_rows<T>(Nk), NR2 = Kind::rows2(Nk2);
    const bool img = p.s != 0.f;                     // uniform
    T* Ks = reinterpret_cast<T*>(smem_x);            // [NR][LD]
    T* Vs = Ks + NR * LD;                            // [NR][LD]
    T* K2s = Vs + NR * LD;                           // [NR2][LD]
    T* V2s = K2s + NR2 * LD;                         // [NR2][LD]
    const int bh = blockIdx.x / p.nchunk, chunk = blockIdx.x % p.nchunk;
    const int b = bh / p.H, h = bh % p.H;
    const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, lg = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    short_stage<T, DP>(Ks, Vs, p.K + b * p.bsk + h * D, p.V + b * p.bsv + h * D, p.ldk, p.ldv, NR, Nk, D, tid, 64 * X2_WAVES);
    if (img) short_stage<T, DP>(K2s, V2s, p.K2 + b * p.bsk2 + h * D, p.V2 + b * p.bsv2 + h * D, p.ldk2, p.ldv2, NR2, Nk2, D, tid, 64 * X2_WAVES);
    __syncthreads();

    const int ntiles = (Nq + 15) >> 4;
    const int t_end = min((chunk + 1) * p.tpb, ntiles);
    const int nsub = (Nk + 15) >> 4, nsub2 = (Nk2 + 15) >> 4;    // sub-tiles with 16 j < Nk (< Nk2)
    const T* qh = p.Q + b * p.bsq + h * D;
    ShortQ<T, DP> qf, qn;
    if constexpr (Kind::Q_PREFETCH) {
#pragma unroll
        for (int s = 0; s < ShortQ<T, DP>::NW; s++) qn.w[s] = zero8();
        qf.load(qh, (chunk * p.tpb + w) * 16 + li, Nq, p.ldq, D, lg);
    }
    for (int tile = chunk * p.tpb + w; tile < t_end; tile += X2_WAVES) {
        const int q = tile * 16 + li;
        if constexpr (Kind::Q_PREFETCH) {
            if (tile + X2_WAVES < t_end) qn.load(qh, (tile + X2_WAVES) * 16 + li, Nq, p.ldq, D, lg);       // uniform
        } else {
            qf.load(qh, q, Nq, p.ldq, D, lg);
        }
        f32x4 sc[SHORT_MAXSUB], sc2[X2_SUB2], acc[DT];
        short_scores<T, DP, SHORT_MAXSUB, false>(sc, Ks, qf, nsub, Nk, p.scale2, 0, li, lg);
        const float l = short_softmax<SHORT_MAXSUB, Kind::FAST_EXP>(sc);
        float l2 = 1.f;
        if (img) {
            short_scores<T, DP, X2_SUB2, false>(sc2, K2s, qf, nsub2, Nk2, p.scale2, 0, li, lg);
            l2 = short_softmax<X2_SUB2, Kind::FAST_EXP>(sc2);
        }
#pragma unroll
        for (int i = 0; i < DT; i++) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (img) {                                   // the image set first: its sum is brought to the text set's normalisation
            short_pv<T, DP, X2_SUB2>(acc, V2s, sc2, NR2 / 16, li, lg);       // every staged sub-tile: bf16 a constant, fp32 = nsub2
            const float f = p.s * l / l2;
#pragma unroll
            for (int i = 0; i < DT; i++) acc[i] *= f;
        }
        short_pv<T, DP, SHORT_MAXSUB>(acc, Vs, sc, nsub, li, lg);
        if (q < Nq) short_store<T, DP>(p.O + b * p.bso + h * D + (long long)q * p.ldo, acc, 1.0f / l, D, lg);
        if constexpr (Kind::Q_PREFETCH) qf = qn;
    }
}

template <typename T, int DP>
size_t x2_lds_bytes(int Nk, int Nk2) { return short_lds_bytes<T, DP>(short_rows<T>(Nk) + Cross2Kind<T>::rows2(Nk2)); }

template <typename T, int DP>
int launch_cross2(const Cross2Params<T>& p, int B, hipStream_t s) {
    const size_t lds = x2_lds_bytes<T, DP>(p.Nk, p.Nk2);
    if (lds > X2_LDS_MAX) return SIDLSG_EINVAL;      // fp32 only: the bf16 maximum is 110 KB
    const size_t most = x2_lds_bytes<T, DP>(X2_MAXN, X2_MAXN2);
    if (const int e = sidlsg_lds_limit<&attn_cross2_kernel<T, DP>>(most < X2_LDS_MAX ? most : X2_LDS_MAX)) return e;
    const dim3 grid((unsigned)((long long)B * p.H * p.nchunk)), block(64 * X2_WAVES);
    SidlsgTraceScope ts(SIDLSG_FAM_ATTN_FWD, 4.0 * B * p.H * (double)p.Nq * (p.Nk + p.Nk2) * p.D,
                        sizeof(T) * B * p.H * (2.0 * p.Nq + 2.0 * p.Nk + 2.0 * p.Nk2) * p.D);
    SIDLSG_LAUNCH((attn_cross2_kernel<T, DP>), grid, block, lds, s, p);
    return sidlsg_last_error();
}

template <typename T>
int attn_cross2_t(const void* Q, const void* K, const void* V, const void* K2, const void* V2, void* O, float sc, bool prescaled, int B, int H,
                  int Nq, int Nk, int Nk2, int D, int ldq, int ldk, int ldv, int ldk2, int ldv2, int ldo, long long bsq, long long bsk,
                  long long bsv, long long bsk2, long long bsv2, long long bso, void* stream) {
    constexpr int DSTEP = sizeof(T) == 2 ? 8 : 4;
    if (B <= 0 || H <= 0 || Nq < 1) return SIDLSG_EINVAL;
    if (Nk < 1 || Nk > X2_MAXN || Nk2 < 1 || Nk2 > X2_MAXN2) return SIDLSG_EINVAL;
    if (D < DSTEP || D > 160 || D % DSTEP) return SIDLSG_EINVAL;
    if (!(sc == sc) || sc - sc != 0.f) return SIDLSG_EINVAL;                     // NaN or infinite scale
    if (!attn_views_ok<T>({{Q, ldq, bsq}, {K, ldk, bsk}, {V, ldv, bsv}, {K2, ldk2, bsk2}, {V2, ldv2, bsv2}, {O, ldo, bso}}, (long long)H * D))
        return SIDLSG_EINVAL;
    const int ntiles = (int)(((long long)Nq + 15) >> 4);
    Cross2Params<T> p;
    p.tpb = ntiles >= 128 ? 4 * X2_WAVES : X2_WAVES;
    p.nchunk = (ntiles + p.tpb - 1) / p.tpb;
    if ((long long)B * H * p.nchunk >= (1LL << 31)) return SIDLSG_EINVAL;
    p.Q = (const T*)Q; p.K = (const T*)K; p.V = (const T*)V; p.K2 = (const T*)K2; p.V2 = (const T*)V2; p.O = (T*)O;
    p.H = H; p.Nq = Nq; p.Nk = Nk; p.Nk2 = Nk2; p.D = D;
    p.ldq = ldq; p.ldk = ldk; p.ldv = ldv; p.ldk2 = ldk2; p.ldv2 = ldv2; p.ldo = ldo;
    p.bsq = bsq; p.bsk = bsk; p.bsv = bsv; p.bsk2 = bsk2; p.bsv2 = bsv2; p.bso = bso;
    p.scale2 = prescaled ? 1.0f : (float)(1.4426950408889634 / sqrt((double)D));
    p.s = sc;
    return attn_width_dispatch<short_tile<T>(), 160>(D, [&](auto dp) { return launch_cross2<T, decltype(dp)::value>(p, B, (hipStream_t)stream); });
}

}  // namespace

extern "C" {

int sidlsg_attn_cross2_fwd(const void* Q, const void* K, const void* V, const void* K2, const void* V2, void* O, float s, int B, int H, int Nq,
                           int Nk, int Nk2, int D, int ldq, int ldk, int ldv, int ldk2, int ldv2, int ldo, long long bsq, long long bsk,
                           long long bsv, long long bsk2, long long bsv2, long long bso, void* stream) {
    return attn_cross2_t<bf16>(Q, K, V, K2, V2, O, s, false, B, H, Nq, Nk, Nk2, D, ldq, ldk, ldv, ldk2, ldv2, ldo, bsq, bsk, bsv, bsk2, bsv2, bso,
                               stream);
}
int sidlsg_attn_cross2_fwd_ps(const void* Q, const void* K, const void* V, const void* K2, const void* V2, void* O, float s, int B, int H, int Nq,
                              int Nk, int Nk2, int D, int ldq, int ldk, int ldv, int ldk2, int ldv2, int ldo, long long bsq, long long bsk,
                              long long bsv, long long bsk2, long long bsv2, long long bso, void* stream) {
    return attn_cross2_t<bf16>(Q, K, V, K2, V2, O, s, true, B, H, Nq, Nk, Nk2, D, ldq, ldk, ldv, ldk2, ldv2, ldo, bsq, bsk, bsv, bsk2, bsv2, bso,
                               stream);
}
int sidlsg_attn_cross2_fwd_f32(const void* Q, const void* K, const void* V, const void* K2, const void* V2, void* O, float s, int B, int H, int Nq,
                               int Nk, int Nk2, int D, int ldq, int ldk, int ldv, int ldk2, int ldv2, int ldo, long long bsq, long long bsk,
                               long long bsv, long long bsk2, long long bsv2, long long bso, void* stream) {
    return attn_cross2_t<float>(Q, K, V, K2, V2, O, s, false, B, H, Nq, Nk, Nk2, D, ldq, ldk, ldv, ldk2, ldv2, ldo, bsq, bsk, bsv, bsk2, bsv2, bso,
                                stream);
}

}  // extern "C"
