// Shared device helpers for the gfx950 (MI355X / CDNA4) kernels of the SiD-LSG hot path.
// wave = 64 lanes; MFMA 16x16x32 bf16; LDS 160 KiB/CU.  No CUDA compatibility shims.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

typedef __bf16 bf16;
typedef bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

#define SIDLSG_OK 0
#define SIDLSG_EINVAL (-22)

#define DEVFN __device__ __forceinline__

DEVFN float bf2f(bf16 x) { return (float)x; }
DEVFN bf16 f2bf(float x) { return (bf16)x; }

DEVFN float silu_f(float x) { return x / (1.0f + __expf(-x)); }
// d/dx [x*sigmoid(x)] = s*(1 + x*(1-s))
DEVFN float silu_grad_f(float x) {
    float s = 1.0f / (1.0f + __expf(-x));
    return s * (1.0f + x * (1.0f - s));
}
DEVFN float gelu_f(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752f)); }
DEVFN float gelu_grad_f(float x) {
    float cdf = 0.5f * (1.0f + erff(x * 0.70710678118654752f));
    float pdf = 0.3989422804014327f * __expf(-0.5f * x * x);
    return cdf + x * pdf;
}

// bf16 activations: exact GELU through erff costs ~34 VALU instructions per element and made the GEGLU kernels VALU-bound
// (3.3 TB/s); Abramowitz-Stegun 7.1.26 (|error| < 5.4e-7 on erf, < 3.7e-7 on gelu -- four orders below a bf16 ulp) needs 14,
// and the exponential it uses is the Gaussian the derivative needs anyway.  The fp32-accurate mode keeps erff.
DEVFN void gelu_fast(float x, float& gelu, float& dgelu) {
    const float ax = fabsf(x) * 0.70710678118654752f;
    const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, ax, 1.0f));
    float p = fmaf(1.061405429f, t, -1.453152027f);
    p = fmaf(p, t, 1.421413741f);
    p = fmaf(p, t, -0.284496736f);
    p = fmaf(p, t, 0.254829592f);
    const float e = __builtin_amdgcn_exp2f(-0.72134752044448170f * x * x);   // exp(-x^2 / 2)
    const float erfv = copysignf(fmaf(-p * t, e, 1.0f), x);                   // erf(x / sqrt 2)
    const float cdf = fmaf(0.5f, erfv, 0.5f);
    gelu = x * cdf;
    dgelu = fmaf(x * 0.3989422804014327f, e, cdf);
}
// SiLU on bf16 activations: v_rcp_f32 (1 ulp) instead of the IEEE division sequence -- 15 -> 6 VALU instructions per element
// forward, 18 -> 8 for the derivative; GroupNorm+SiLU applies it to every element it streams.  fp32 mode keeps the division.
DEVFN float sigmoid_fast(float x) { return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * x)); }
template <typename T> DEVFN float silu_t(float x) { return silu_f(x); }
template <> DEVFN float silu_t<bf16>(float x) { return x * sigmoid_fast(x); }
template <typename T> DEVFN float silu_grad_t(float x) { return silu_grad_f(x); }
template <> DEVFN float silu_grad_t<bf16>(float x) { const float s = sigmoid_fast(x); return s * fmaf(x, 1.0f - s, 1.0f); }
template <typename T> DEVFN float gelu_t(float x) { return gelu_f(x); }
template <> DEVFN float gelu_t<bf16>(float x) { float g, d; gelu_fast(x, g, d); return g; }
template <typename T> DEVFN void gelu_pair_t(float x, float& g, float& d) { g = gelu_f(x); d = gelu_grad_f(x); }
template <> DEVFN void gelu_pair_t<bf16>(float x, float& g, float& d) { gelu_fast(x, g, d); }

DEVFN float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
DEVFN float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// XCD-contiguous block numbering.  Hardware block b runs on XCD b % 8; the renumbering gives every XCD a contiguous range of the
// nblk logical blocks, so blocks that share an operand panel (a GEMM's A row-panel, an attention head's K / V, a GroupNorm sample)
// sit on one XCD and meet in its L2.  I: int, or unsigned where the caller's ids are.
template <typename I>
DEVFN I xcd_contiguous(I bid, I nblk) {
    const I q = nblk >> 3, r = nblk & 7, xcd = bid & 7, idx = bid >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

// 16-byte global load/store of 8 bf16
DEVFN bf16x8 ld8(const bf16* p) { return *reinterpret_cast<const bf16x8*>(p); }
DEVFN void st8(bf16* p, bf16x8 v) { *reinterpret_cast<bf16x8*>(p) = v; }
DEVFN bf16x8 zero8() {
    u32x4 z = {0u, 0u, 0u, 0u};
    return __builtin_bit_cast(bf16x8, z);
}

// 8 consecutive activation elements as fp32 registers.  The kernels are templated on the activation storage type T:
// bf16 (production: 16 bytes per lane) or float (the fp32-accurate parity mode: two 16-byte accesses per lane).
template <typename T> DEVFN void ldv8(const T* p, float (&v)[8]);
template <> DEVFN void ldv8<bf16>(const bf16* p, float (&v)[8]) {
    const bf16x8 t = ld8(p);
#pragma unroll
    for (int e = 0; e < 8; e++) v[e] = bf2f(t[e]);
}
template <> DEVFN void ldv8<float>(const float* p, float (&v)[8]) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
    v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3]; v[4] = b[0]; v[5] = b[1]; v[6] = b[2]; v[7] = b[3];
}
// 8 consecutive activation elements as they are in memory (no conversion: the registers are not touched until unpack(), so a
// load can stay in flight across control flow and stores -- see the prefetching row loops of norm.hip)
template <typename T> struct Raw8;
template <> struct Raw8<bf16> {
    bf16x8 v;
    DEVFN void load(const bf16* p) { v = ld8(p); }
    DEVFN void unpack(float (&o)[8]) const {
#pragma unroll
        for (int e = 0; e < 8; e++) o[e] = bf2f(v[e]);
    }
};
template <> struct Raw8<float> {
    f32x4 a, b;
    DEVFN void load(const float* p) { a = *reinterpret_cast<const f32x4*>(p); b = *reinterpret_cast<const f32x4*>(p + 4); }
    DEVFN void unpack(float (&o)[8]) const { o[0] = a[0]; o[1] = a[1]; o[2] = a[2]; o[3] = a[3]; o[4] = b[0]; o[5] = b[1]; o[6] = b[2]; o[7] = b[3]; }
};
// Branch-free predicated accesses through a buffer descriptor: an offset >= SIDLSG_OOB is out of range for every descriptor
// (< 2 GiB of records), so the load returns zeros and the store is dropped -- no `if (valid)` around the access.  That matters beyond
// the saved branch: gfx950 retires loads and stores through ONE in-order counter and the compiler merges the counter state of the two
// arms of a branch conservatively, so a store inside a divergent `if` turns every later counted wait into s_waitcnt vmcnt(0), i.e. a
// prefetched load can no longer be waited for without also waiting for the stores issued behind it.
constexpr unsigned SIDLSG_OOB = 0x80000000u;
DEVFN __amdgpu_buffer_rsrc_t mk_buf(const void* p, long long bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, (int)(bytes > 0x7FFFFFFFll ? 0x7FFFFFFFll : bytes), 0x00020000);
}
DEVFN void Raw8_bload(Raw8<bf16>& r, __amdgpu_buffer_rsrc_t rs, unsigned elem) {
    r.v = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rs, elem >= SIDLSG_OOB ? elem : elem * 2u, 0, 0));
}
DEVFN void Raw8_bload(Raw8<float>& r, __amdgpu_buffer_rsrc_t rs, unsigned elem) {
    const unsigned o = elem >= SIDLSG_OOB ? elem : elem * 4u;
    r.a = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, o, 0, 0));
    r.b = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, o, 16, 0));
}
// 8 consecutive outputs at ELEMENT index `elem` (or SIDLSG_OOB: dropped) of a [..][C] tensor of T, or (F8) of e4m3 bytes
template <typename T, bool F8> DEVFN void bst8_out(__amdgpu_buffer_rsrc_t rs, unsigned elem, const float (&v)[8]);
template <typename T> DEVFN void stv8(T* p, const float (&v)[8]);
template <> DEVFN void stv8<bf16>(bf16* p, const float (&v)[8]) {
    bf16x8 o;
#pragma unroll
    for (int e = 0; e < 8; e++) o[e] = f2bf(v[e]);
    st8(p, o);
}
template <> DEVFN void stv8<float>(float* p, const float (&v)[8]) {
    *reinterpret_cast<f32x4*>(p) = (f32x4){v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f32x4*>(p + 4) = (f32x4){v[4], v[5], v[6], v[7]};
}

// ---- OCP e4m3 output (frozen networks: activations written as e4m3 at unit scale for the MX-fp8 contractions) ----
// explicit clamp to the e4m3 range (v_med3_f32): whether v_cvt_pk_fp8_f32 saturates or returns NaN past +-448 depends on a
// mode bit this library does not own.  A NaN input stays NaN (the conversion turns it into an e4m3 NaN byte): the clamp is the
// IEEE 754-2019 maximum / minimum pair (v_maximum3_f32, v_minimum3_f32 on gfx950), which propagate NaN.  v_med3_f32 -- one
// instruction less -- returns the smaller bound or the larger by the NaN's sign instead, so a NaN activation became +-448.
DEVFN float clamp_e4m3(float x) { return __builtin_elementwise_minimum(__builtin_elementwise_maximum(x, -448.f), 448.f); }
DEVFN unsigned cvt4_fp8(float a, float b, float c, float d) {
    a = clamp_e4m3(a); b = clamp_e4m3(b); c = clamp_e4m3(c); d = clamp_e4m3(d);
    int r = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
    r = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, r, true);
    return (unsigned)r;
}
// 8 consecutive outputs at element index `idx` of y: T elements, or (F8) e4m3 bytes in the same [..][C] geometry
template <typename T, bool F8>
DEVFN void st8_out(T* y, size_t idx, const float (&v)[8]) {
    if constexpr (F8) {
        u32x2 q = {cvt4_fp8(v[0], v[1], v[2], v[3]), cvt4_fp8(v[4], v[5], v[6], v[7])};
        *reinterpret_cast<u32x2*>(reinterpret_cast<unsigned char*>(y) + idx) = q;
    } else {
        stv8<T>(y + idx, v);
    }
}
template <typename T, bool F8> DEVFN void bst8_out(__amdgpu_buffer_rsrc_t rs, unsigned elem, const float (&v)[8]) {
    const bool oob = elem >= SIDLSG_OOB;
    if constexpr (F8) {
        const u32x2 q = {cvt4_fp8(v[0], v[1], v[2], v[3]), cvt4_fp8(v[4], v[5], v[6], v[7])};
        __builtin_amdgcn_raw_buffer_store_b64(q, rs, elem, 0, 0);
    } else if constexpr (sizeof(T) == 2) {
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 8; e++) o[e] = f2bf(v[e]);
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), rs, oob ? elem : elem * 2u, 0, 0);
    } else {
        const unsigned o = oob ? elem : elem * 4u;
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, (f32x4){v[0], v[1], v[2], v[3]}), rs, o, 0, 0);
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, (f32x4){v[4], v[5], v[6], v[7]}), rs, o, 16, 0);
    }
}
template <typename T> DEVFN void zerov8(T* p) {
    const float z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    stv8<T>(p, z);
}

// ---- in-library kernel timing (trace.hip): families of the step's kernels, and the launch macro every family kernel goes through
enum { SIDLSG_FAM_GEMM = 0, SIDLSG_FAM_CONV, SIDLSG_FAM_ATTN_FWD, SIDLSG_FAM_ATTN_BWD, SIDLSG_FAM_WGRAD, SIDLSG_FAM_CONV_WGRAD,
       SIDLSG_FAM_GN_FWD, SIDLSG_FAM_GN_BWD, SIDLSG_FAM_LN_FWD, SIDLSG_FAM_LN_BWD, SIDLSG_TRACE_FAMILIES };
bool sidlsg_trace_scope_begin(int family, double work, double bytes);
void sidlsg_trace_scope_end();
bool sidlsg_trace_events(hipEvent_t* e0, hipEvent_t* e1);
#ifdef SIDLSG_EXP_SKIP      // measurement build only (tools/ab/build_skip_variant.sh): the kernels of the families in $SIDLSG_EXP_SKIP_FAMILIES (bit mask)
#include <cstdlib>          // are not launched -- WRONG results; the step-time difference is the family's exposed cost (tools/family_exposed_cost.sh)
inline thread_local int sidlsg_cur_family = -1;
static inline bool sidlsg_exp_skip() {
    static const long mask = getenv("SIDLSG_EXP_SKIP_FAMILIES") ? strtol(getenv("SIDLSG_EXP_SKIP_FAMILIES"), nullptr, 0) : 0;
    return sidlsg_cur_family >= 0 && ((mask >> sidlsg_cur_family) & 1);
}
#define SIDLSG_SKIP_CHECK if (sidlsg_exp_skip()) break;
#else
#define SIDLSG_SKIP_CHECK
#endif
struct SidlsgTraceScope {
    bool open;
    SidlsgTraceScope(int family, double work, double bytes = 0.0) : open(sidlsg_trace_scope_begin(family, work, bytes)) {
#ifdef SIDLSG_EXP_SKIP
        sidlsg_cur_family = family;
#endif
    }
    ~SidlsgTraceScope() {
        if (open) sidlsg_trace_scope_end();
#ifdef SIDLSG_EXP_SKIP
        sidlsg_cur_family = -1;
#endif
    }
};
#include <hip/hip_ext.h>
// hipLaunchKernelGGL, or -- inside a sampled trace scope -- the same launch with start / stop events bound to ITS dispatch packet
#define SIDLSG_LAUNCH(kern, grid, block, lds, stream, ...)                                                     \
    do {                                                                                                        \
        SIDLSG_SKIP_CHECK                                                                                       \
        hipEvent_t te0_, te1_;                                                                                  \
        if (sidlsg_trace_events(&te0_, &te1_)) hipExtLaunchKernelGGL(kern, grid, block, lds, stream, te0_, te1_, 0, __VA_ARGS__); \
        else hipLaunchKernelGGL(kern, grid, block, lds, stream, __VA_ARGS__);                                   \
    } while (0)

// Launch-error helper for the extern "C" entry points: returns the HIP error code (0 = ok).
static inline int sidlsg_last_error() { return (int)hipGetLastError(); }

// Raises KERNEL's dynamic-LDS limit to `bytes` -- the most that kernel can ask for -- on its first launch.  0, or the HIP error.
template <auto KERNEL>
int sidlsg_lds_limit(size_t bytes) {
    static bool done = false;                        // per kernel instantiation
    if (!done) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) {
            const int e = (int)hipGetLastError();
            return e ? e : (int)hipErrorUnknown;
        }
        done = true;
    }
    return 0;
}

// Environment switches of the host launchers (read once: every site keeps its `static const`).  A number: the variable's atoi, `dflt`
// when unset.  An on-by-default switch: off only when the variable is set and its atoi is 0; an off-by-default one: env_int(name, 0) != 0.
static inline int sidlsg_env_int(const char* name, int dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}
static inline bool sidlsg_env_on(const char* name) { return sidlsg_env_int(name, 1) != 0; }

// ---- library state (state.hip)
// Deterministic mode (sidlsg_set_deterministic): every parameter-gradient reduction takes an order-fixed form,
// so its bits depend only on the inputs and the launch configuration.  Off: the atomic forms of the fast path.
bool sidlsg_det();
// The split-K / pixel-split scratch of stream `s` (sidlsg_set_stream_workspace, else sidlsg_set_workspace); null / 0 when none.
float* sidlsg_ws_for_stream(hipStream_t s, long long* bytes);
