// Library-wide state of libsidlsg_hip.so: the split-K / pixel-split workspaces, the deterministic flag, the dispatch record, the p8 mode
// and the split-K rule, with their C entry points.  Host code only.  Declared in common.h (sidlsg_det, sidlsg_ws_for_stream: norm.hip and
// the other reductions use them) and in gemm_core.h (what only the contraction units reach).
#include "gemm_core.h"

// Split-K / pixel-split scratch.  The default workspace (sidlsg_set_workspace) serves every stream that has no workspace
// of its own; a stream that runs contractions CONCURRENTLY with another one (the teacher evaluated beside the fake-score
// network, sid_step.py) registers a private one with sidlsg_set_stream_workspace, so the two never share slabs.
struct WsSlot { hipStream_t stream; float* ptr; long long bytes; };
static float* g_ws_default = nullptr;
static long long g_ws_default_bytes = 0;
static WsSlot g_ws_slots[8] = {};
static int g_ws_nslots = 0;
Ws ws_for(hipStream_t s) {
    for (int i = 0; i < g_ws_nslots; i++)
        if (g_ws_slots[i].stream == s) return {g_ws_slots[i].ptr, g_ws_slots[i].bytes};
    return {g_ws_default, g_ws_default_bytes};
}
float* sidlsg_ws_for_stream(hipStream_t s, long long* bytes) {
    const Ws w = ws_for(s);
    *bytes = w.ptr ? w.bytes : 0;
    return w.ptr;
}

// Deterministic mode: -2 = not read yet (SIDLSG_DETERMINISTIC), else 0 / 1.  Process-wide, like g_p8_mode.
static int g_det_mode = -2;
bool sidlsg_det() {
    if (g_det_mode == -2) g_det_mode = sidlsg_env_int("SIDLSG_DETERMINISTIC", 0) ? 1 : 0;
    return g_det_mode == 1;
}

thread_local LaunchRecord g_last_launch = {};      // the dispatch record (gemm_core.h: record_launch and its kin write it inline)

// The split-K rule of every GEMM launcher: a launch of few tiles with a long contraction splits K so that ~TARGET blocks exist.
// tiles: output tiles of the unsplit launch; nk: its k-tiles; mn = M * N (one fp32 slab per split in the workspace `w`, at least two must
// fit); min_nk: k-tiles from which a contraction is split at all; min_kt: k-tiles every split keeps.  Returns the split count, 1 = none.
int splitk_splits(long long tiles, int nk, long long mn, const Ws& w, int min_nk, int min_kt) {
    static const int MIN_TILES = sidlsg_env_int("SIDLSG_GEMM_MIN_TILES", 384);     // A/B knobs (defaults = the measured best)
    static const int TARGET = sidlsg_env_int("SIDLSG_SPLITK_TARGET", 512);          // blocks a split launch aims at (2 per CU)
    if (tiles >= MIN_TILES || nk < min_nk || !w.ptr || mn * 8 > w.bytes) return 1;
    const long long splits = std::min(std::min<long long>((TARGET + tiles - 1) / tiles, w.bytes / (mn * 4)), (long long)std::min(nk / min_kt, 16));
    return splits >= 2 ? (int)splits : 1;
}
// The bf16 kernels (64-element k-tiles): split from MIN_NK k-tiles on, keeping at least MIN_KT per split (A/B knobs)
int splitk_splits_bf16(long long tiles, int nk, long long mn, const Ws& w) {
    static const int MIN_NK = sidlsg_env_int("SIDLSG_SPLITK_MIN_NK", 32);
    static const int MIN_KT = sidlsg_env_int("SIDLSG_SPLITK_MIN_KT", 8);
    return splitk_splits(tiles, nk, mn, w, MIN_NK, MIN_KT);
}

static int g_p8_mode = -2;        // -2: not read yet
int p8_mode() {
    if (g_p8_mode == -2) g_p8_mode = sidlsg_env_int("SIDLSG_GEMM_P8", -1);
    return g_p8_mode;
}

extern "C" {

// Deterministic mode: 1 on, 0 off, -1 query only.  Returns the previous setting.  See include/sidlsg_hip.h.
int sidlsg_set_deterministic(int on) {
    const int old = sidlsg_det() ? 1 : 0;
    if (on >= 0) g_det_mode = on ? 1 : 0;
    return old;
}

// (A/B switch) which GEMM / conv calls take the 256-row-tile kernels of gemm_p8.h: -1 by rule (default), 0 never, 1 / 2 every
// admissible call on the 256 x 160 / 256 x 320 configuration.  Returns the previous setting.
int sidlsg_debug_set_p8(int mode) {
    const int old = p8_mode();
    g_p8_mode = mode;
    return old;
}

// (diagnostic) the dispatch record of the calling thread's last GEMM / conv / weight-gradient call: see include/sidlsg_hip.h
int sidlsg_debug_last_launch(int* out, int n) {
    if (!out || n < 1) return SIDLSG_EINVAL;
    const int m = std::min(n, (int)SIDLSG_REC_INTS);
    for (int i = 0; i < m; i++) out[i] = g_last_launch.v[i];
    return m;
}

// Optional scratch for split-K GEMMs and weight gradients: `ptr` = device memory of `bytes` bytes, owned by the
// caller, used by every later sidlsg_gemm_bf16 / sidlsg_conv3x3_bf16 call of this process (one stream at a time).
// Pass NULL/0 to disable split-K.
int sidlsg_set_workspace(void* ptr, long long bytes) {
    g_ws_default = (float*)ptr; g_ws_default_bytes = ptr ? bytes : 0;
    return SIDLSG_OK;
}

// Private scratch for one stream (see WsSlot).  ptr = NULL removes the entry.  At most 4 streams.
int sidlsg_set_stream_workspace(void* stream, void* ptr, long long bytes) {
    hipStream_t s = (hipStream_t)stream;
    for (int i = 0; i < g_ws_nslots; i++)
        if (g_ws_slots[i].stream == s) {
            if (ptr) { g_ws_slots[i].ptr = (float*)ptr; g_ws_slots[i].bytes = bytes; }
            else { g_ws_slots[i] = g_ws_slots[--g_ws_nslots]; }
            return SIDLSG_OK;
        }
    if (!ptr) return SIDLSG_OK;
    if (g_ws_nslots >= 8) return SIDLSG_EINVAL;
    g_ws_slots[g_ws_nslots++] = {s, (float*)ptr, bytes};
    return SIDLSG_OK;
}

}  // extern "C"
