/* sidlsg_hip.h -- C ABI of libsidlsg_hip.so: the MI355X (gfx950) kernels of the SiD-LSG
 * distillation inner step.  Plain pointers and sizes only (device pointers unless noted);
 * `stream` is a hipStream_t passed as void*.  Every function returns 0 on success, a positive
 * hipError_t if the launch failed, or -22 (EINVAL) if the arguments violate the stated
 * constraints.  No function allocates, synchronises or touches the host heap, so all of them may
 * be captured into a HIP graph.
 *
 * What each entry point replaces in the reference (paths relative to mingyuanzhou/SiD-LSG):
 * the reference has no native code on this path -- every op below is executed there by
 * diffusers/ATen kernels reached through `unet(...).sample` (training/sid_sd_util.py:184,194,
 * 245,263), `torch.optim.Adam.step` (training/sid_training_loop.py:462,549) and inline torch
 * expressions in the loop.  Its only native-operator seam is the plugin API of
 * torch_utils/custom_ops.py:46 + torch_utils/ops/bias_act.cpp:32-97, which sidlsg_bias_act
 * mirrors.  Activations are NHWC bf16 ([tokens][channels], channels contiguous); conv weights
 * are [Cout][3][3][Cin] (= torch channels_last storage of the diffusers [Cout][Cin][3][3]
 * parameter); parameters, statistics, losses and gradients of parameters are fp32.
 */
#ifndef SIDLSG_HIP_H
#define SIDLSG_HIP_H
#ifdef __cplusplus
extern "C" {
#endif

/* epilogue flags of the GEMM / conv entry points */
#define SIDLSG_OUT_F32 1 /* C is fp32 instead of bf16 */
#define SIDLSG_SILU 2    /* y = silu(...) */
#define SIDLSG_ACCUM 4   /* C += ... (fp32 only) */

/* ---- contractions (MFMA bf16 -> fp32) ------------------------------------------------------
 * torch.nn.functional.linear / conv2d(k=1) inside diffusers Attention / FeedForward /
 * Transformer2DModel / ResnetBlock2D.time_emb_proj / conv_shortcut (call site sid_sd_util.py:184).
 * C[M][ldc] = act(alpha * A[M][K] W[N][K]^T + bias[N] + rowvec[m/rows_per_batch][ld_rowvec] + res[M][ldres])
 * K, lda multiples of 8.  bias/res/rowvec may be NULL; ld_rowvec <= 0 means N (a slice of a wider matrix otherwise).
 * Operand contract (this entry point, sidlsg_conv3x3_bf16, their _g2 / _fp8w / _mx8 forms; SIDLSG_EINVAL otherwise): row strides in
 * elements of the operand's type; lda >= K (conv: ldx >= Cin), ldc >= N, ldres >= N, ld_rowvec >= N when given.  C, res and the operands
 * may be views into wider buffers: only columns [0, N) of rows [0, M) are written, nothing else of C is touched, and only columns
 * [0, K) / [0, N) of A / res are read.  N % 8 == 0 selects the vector epilogue, which moves 16 bytes per access (8 bf16 or 4 fp32, at
 * column offsets that are multiples of 8 resp. 4): then C, res, rowvec, bias (and bias1) must be 16-byte aligned, ldc and ldres
 * multiples of 8 (ldc of 4 for an fp32 C) and ld_rowvec a multiple of 4.  Any other N takes an element-wise epilogue without these. */
int sidlsg_gemm_bf16(const void* A, int lda, const void* W, void* C, int ldc, const float* bias, const void* res, int ldres,
                     const float* rowvec, int ld_rowvec, int rows_per_batch, int M, int N, int K, float alpha, int flags,
                     void* stream);

/* torch conv2d(k=3, pad=1, stride 1|2) of ResnetBlock2D.conv1/conv2, Downsample2D, Upsample2D
 * (ups=1 fuses the nearest x2 interpolate), conv_in/conv_out.  X: [B][Hs][Ws][ldx] with the virtual
 * (post-upsample) size H x Wd; W: [Cout][3][3][Cin]; Y: [B][Ho][Wo][ldc].  Same epilogue as the GEMM;
 * rowvec is the per-sample time-embedding projection [B][ld_rowvec] (all ResBlocks' projections come out of ONE GEMM;
 * each conv reads its column slice).  Cin, ldx multiples of 8.
 * The backward-data pass is the same entry point fed with dY and the transposed/flipped weights
 * made by sidlsg_transpose_w. */
int sidlsg_conv3x3_bf16(const void* X, int ldx, const void* W, void* Y, int ldc, const float* bias, const void* res, int ldres,
                        const float* rowvec, int ld_rowvec, int B, int H, int Wd, int Cin, int Cout, int stride, int ups,
                        float alpha, int flags, void* stream);

/* diffusers GEGLU (`FeedForward.net[0]`: proj -> chunk(2) -> hidden * gelu(gate)) with its projection, in ONE kernel: the GEMM's
 * output tile holds 80 features of the value half and the same 80 features of the gate half, so the epilogue emits
 * Y[M][F] = h[:, :F] * gelu(h[:, F:]) next to h[M][N2] = A W^T + bias (N2 = 2 F).  h is what the backward needs (sidlsg_geglu_bwd);
 * H = NULL skips it (a pass without backward).  Y is computed from the bf16-rounded h: bit for bit sidlsg_geglu_fwd(h).  Saves the
 * separate GEGLU pass over h (335 MB read at the 64x64 stage of SD1.5, batch 16).  sidlsg_gemm_geglu_ok: host query -- the fused kernel
 * takes a shape only where the direct-to-LDS GEMM would be dispatched without split-K. */
int sidlsg_gemm_geglu_ok(int M, int N2, int K);
int sidlsg_gemm_geglu_bf16(const void* A, int lda, const void* W, void* H, int ldh, void* Y, int ldy, const float* bias, int M, int N2,
                           int K, void* stream);

/* The backward of the same block (diffusers `FeedForward`: net[2] = Linear(4C -> C) after the GEGLU): data gradient of the FF-out
 * projection with the GEGLU derivative in its epilogue -- dy = dOut Wt^T (Wt [F][K]: the backward-data operand of the [K][F] FF-out
 * weight) stays in the output tile (rounded to bf16 there: bit for bit what sidlsg_geglu_bwd computes from a stored dy),
 * dH[:, :F] = dy * gelu(h[:, F:]), dH[:, F:] = dy * h[:, :F] * gelu'(h[:, F:]); H, dH: [M][ldh], ldh >= 2 F.  Saves the write and
 * the re-read of dy [M][F] (2 x 168 MB at the 64x64 stage of SD1.5, batch 16) and one launch.  autograd reaches it through
 * `loss.backward()` (sid_training_loop.py:450,533).  sidlsg_gemm_geglu_bwd_ok: host query, same admission rule as the forward. */
int sidlsg_gemm_geglu_bwd_ok(int M, int F, int K);
int sidlsg_gemm_geglu_bwd_bf16(const void* dOut, int lda, const void* Wt, const void* H, void* dH, int ldh, int M, int F, int K,
                               void* stream);
/* Grouped variants of the two GEGLU fusions (two frozen networks of one shape on one stacked batch, M even: rows [0, M/2) are contracted
 * with (W, bias) / Wt, rows [M/2, M) with (W1, bias1) / Wt1; otherwise as the single-set entry points above).  The grouped frozen pass of
 * phase B (sid_training_loop.py:494-506: fake-score network and teacher evaluate the same images) takes its FeedForward blocks through
 * these; its backward is the data gradient only. */
int sidlsg_gemm_geglu_bf16_g2(const void* A, int lda, const void* W, const void* W1, void* H, int ldh, void* Y, int ldy, const float* bias,
                              const float* bias1, int M, int N2, int K, void* stream);
int sidlsg_gemm_geglu_bwd_bf16_g2(const void* dOut, int lda, const void* Wt, const void* Wt1, const void* H, void* dH, int ldh, int M, int F,
                                  int K, void* stream);

/* Optional fp32 scratch (device memory owned by the caller): per-split partial-sum slabs for split-K GEMMs/convs with few
 * output tiles and long K (8x8 / 16x16 stages) and for the pixel-split weight gradients (without it they fall back to
 * fp32 atomics, ~2-3x slower on MI355X).  Default for every stream without a private workspace (below): launches sharing
 * it must be ordered on one stream.  NULL disables. */
int sidlsg_set_workspace(void* ptr, long long bytes);
/* A private workspace for launches on `stream` (ptr = NULL removes it; at most 4): needed when two streams run
 * contractions concurrently -- the teacher beside the fake-score network in phase B of the step. */
int sidlsg_set_stream_workspace(void* stream, void* ptr, long long bytes);

/* weight gradients (autograd of the two ops above in the reference: loss.backward(),
 * sid_training_loop.py:450,533).  dW[N][K] += dY[M][N]^T A[M][K] in fp32 (pixel-split partial sums, reduced through the
 * workspace).  dBias (may be NULL): dBias[N] += sum_m dY[m][N], the bias gradient of the same layer, produced by the
 * same kernel (one extra MFMA against a vector of ones per dY fragment) instead of a separate column-sum pass. */
int sidlsg_wgrad_bf16(const void* dY, int ldy, const void* A, int lda, float* dW, float* dBias, int M, int N, int K,
                      void* stream);
/* The same with dW = (not +=), dBias still +=: for gradient storage whose previous contents are dead.  The fused optimizer
 * (sidlsg_adam_ema, zero_grad = 0 on the weight ranges) leaves the weight gradients of a network un-zeroed and the first weight
 * gradient after it overwrites them: 4 B / parameter of zero stores and 4 B / parameter of dW reads less per optimizer step.  Same
 * summation order as the accumulating entry points on a zeroed dW: bit-identical results. */
int sidlsg_wgrad_assign_bf16(const void* dY, int ldy, const void* A, int lda, float* dW, float* dBias, int M, int N, int K,
                             void* stream);
/* Several dense weight gradients as ONE launch + one slab-reduction launch (round 5: the C x C projections of a transformer block each
 * need ~56 pixel splits to fill the chip alone; grouped, the group fills it with ~6 each).  jobs: HOST array of njobs <= 8 records of
 * 64 bytes  { const void* dY; const void* A; float* dW; float* dBias; int ldy, lda, M, N, K, assign; int pad[2]; }  with the meaning
 * of sidlsg_wgrad_bf16 (assign = 0) / sidlsg_wgrad_assign_bf16 (assign = 1) per record; N, K, ldy, lda % 8 == 0, 16-byte aligned operands.
 * The dW of the records of one call must be DISTINCT buffers (the jobs run as one grid: two jobs on one dW would race). */
int sidlsg_wgrad_group_bf16(const void* jobs, int njobs, void* stream);
int sidlsg_wgrad_group160_bf16(const void* jobs, int njobs, void* stream); /* the same on 160 x 160 tiles: every N and K a multiple of 160 */
int sidlsg_conv3x3_wgrad_assign_bf16(const void* dY, int ldy, const void* X, int ldx, float* dW, float* dBias, int B, int H, int Wd,
                                     int Cin, int Cout, int stride, int ups, void* stream);
int sidlsg_debug_wgrad_blocks_per_cu(int which); /* host diagnostic: resident blocks per CU of the weight-gradient kernels (0: 128x128, 1: 160x128, 2: 160x160 tiles) */
int sidlsg_debug_set_p8(int mode); /* A/B switch: which GEMM / conv calls take the 256-row-tile kernels (csrc/gemm_p8.h): -1 by rule (default), 0 never, 1 / 2 always the 256x160 / 256x320 configuration when admissible; returns the previous setting */
int sidlsg_conv3x3_wgrad_bf16(const void* dY, int ldy, const void* X, int ldx, float* dW, float* dBias, int B, int H, int Wd,
                              int Cin, int Cout, int stride, int ups, void* stream);

/* ---- dispatch record (host diagnostic; tests/gemm_cases.py) ----------------------------------
 * Which kernel a GEMM / conv / weight-gradient entry point chose.  Every host launcher of csrc/gemm.hip, gemm_fp8.hip, wgrad.hip and gemm_p8.h writes a
 * thread-local record of SIDLSG_REC_INTS ints just before it launches: a handful of plain stores, no HIP call, nothing about the
 * launch changes.  The record is written BEFORE the launch, so it is there also when the launch itself fails (no device).
 * sidlsg_debug_last_launch copies the record of the calling thread's last such call: out[SIDLSG_REC_*], at most n ints; returns
 * the number of ints copied, or SIDLSG_EINVAL for a NULL out or n < 1.  A call that was rejected with SIDLSG_EINVAL before its
 * launcher leaves the record of the call before it; SIDLSG_REC_SEQ counts the records written by the thread, so a caller can tell.
 * The numbers below are part of the ABI (tests parse them from this header): add at the end, never renumber. */
enum sidlsg_kernel_id {
    SIDLSG_K_NONE = 0,                /* no launcher has run on this thread yet */
    SIDLSG_K_GEMM_BF16 = 1,           /* gemm_bf16_kernel<BM, BN, MODE, PAD>: register-staged tiles */
    SIDLSG_K_GEMM_V3 = 2,             /* gemm_v3_kernel<MODE>: 128 x 160, direct-to-LDS (also under the GEGLU fusions) */
    SIDLSG_K_GEMM_P8S = 3,            /* gemm_p8s_kernel<MODE>: 256 x 160 */
    SIDLSG_K_GEMM_P8W = 4,            /* gemm_p8w_kernel<MODE>: 256 x 320 */
    SIDLSG_K_GEMM_P8W_GEGLU = 5,      /* gemm_p8w_geglu_kernel */
    SIDLSG_K_GEMM_P8W_GEGLU_BWD = 6,  /* gemm_p8w_geglu_bwd_kernel */
    SIDLSG_K_GEMM_AS = 7,             /* gemm_as_kernel<5, RES>: A-stationary, K = 320 */
    SIDLSG_K_GEMM_MX8 = 8,            /* gemm_mx8_kernel<MODE>: e4m3 x e4m3 */
    SIDLSG_K_GEMM_FP8W = 9,           /* gemm_fp8w_kernel<MODE>: bf16 x e4m3 weights */
    SIDLSG_K_WGRAD_BF16 = 10,         /* wgrad_bf16_kernel<MODE>: unaligned operands */
    SIDLSG_K_WGRAD_V2 = 11,           /* wgrad_v2_kernel<MODE>: 128 x 128 */
    SIDLSG_K_WGRAD_V2W = 12,          /* wgrad_v2w_kernel<MODE>: 160 x 128 */
    SIDLSG_K_WGRAD_V2F = 13,          /* wgrad_v2f_kernel: conv, 128 x 128, constant-advance gather */
    SIDLSG_K_WGRAD_V2WF = 14,         /* wgrad_v2wf_kernel: conv, 160 x 128, constant-advance gather */
    SIDLSG_K_WGRAD_V2S = 15,          /* wgrad_v2s_kernel: dense, 160 x 160 */
    SIDLSG_K_WGRAD_V2G = 16,          /* wgrad_v2g_kernel: grouped dense, 128 x 128 */
    SIDLSG_K_WGRAD_V2SG = 17          /* wgrad_v2sg_kernel: grouped dense, 160 x 160 */
};
enum sidlsg_launch_record {
    SIDLSG_REC_KERNEL = 0,  /* enum sidlsg_kernel_id */
    SIDLSG_REC_BM = 1,      /* tile rows (weight gradients: tile extent along N) */
    SIDLSG_REC_BN = 2,      /* tile columns (weight gradients: tile extent along K) */
    SIDLSG_REC_MODE = 3,    /* the kernel's MODE: GEMM family 0 dense, 1 conv with Cin % 64 == 0, 2 any conv; weight gradients 0 dense, 1 conv */
    SIDLSG_REC_PAD = 4,     /* gemm_bf16_kernel's PAD (1: pad 1 on all sides, 0: bottom / right only); -1 for every other kernel */
    SIDLSG_REC_P8 = 5,      /* p8 configuration: 0 = 256 x 160, 1 = 256 x 320; -1: not a p8 kernel */
    SIDLSG_REC_SPLITS = 6,  /* K splits (GEMM / conv) or pixel splits (weight gradients; a grouped launch: the largest of its jobs); 1 = none */
    SIDLSG_REC_PARTIAL = 7, /* where partial sums went: SIDLSG_PART_* */
    SIDLSG_REC_FINISH = 8,  /* kernels that followed: bit mask of SIDLSG_FIN_* */
    SIDLSG_REC_SEQ = 9,     /* records written by this thread so far, this one included */
    SIDLSG_REC_INTS = 10
};
enum sidlsg_launch_partial { SIDLSG_PART_ONE = 0 /* one split: the kernel finishes its output */, SIDLSG_PART_SLABS = 1 /* fp32 slabs in the workspace */,
                             SIDLSG_PART_ATOMICS = 2 /* fp32 atomics onto the output */ };
enum sidlsg_launch_finish { SIDLSG_FIN_GEMM = 1 /* gemm_finish_kernel */, SIDLSG_FIN_WGRAD_REDUCE = 2 /* wgrad_reduce(_g)_kernel */,
                            SIDLSG_FIN_COLSUM = 4 /* deterministic mode: the bias gradient as a column sum of dY */ };
int sidlsg_debug_last_launch(int* out, int n);

/* ---- deterministic mode --------------------------------------------------------------------
 * Process-wide switch (like sidlsg_debug_set_p8); initial value from the environment variable SIDLSG_DETERMINISTIC (unset or 0: off).
 * On, every reduction of this library gives bits that depend only on its inputs and its launch configuration -- never on block
 * scheduling or stream timing.  What changes while it is on (off: nothing does):
 *   - column sums (sidlsg_colsum*, incl. _strided and _f32): per-chunk totals go to a slab [B][chunks][N] in the stream's workspace
 *     (sidlsg_set_stream_workspace, else sidlsg_set_workspace) and a second kernel adds them in ascending chunk, then batch order;
 *     without a workspace: one chunk per batch for per_batch and one chunk over all rows for total (slow, order-fixed);
 *   - LayerNorm / GroupNorm dgamma, dbeta: the partial-sum reduction runs with one thread per channel over all partials in order,
 *     immediate and deferred (sidlsg_flush_reductions) alike, so the two give equal bits; a GroupNorm backward WITH parameter
 *     gradients skips the one-pass (small-stage) and per-group (SIDLSG_GN_GROUP) kernels, which add per block with atomics, and
 *     takes the two-kernel path;
 *   - bf16 weight gradients (single, grouped, dense, conv): pixel splits only with a slab per split (else one split); with several
 *     splits the bias gradient is a column sum of dY (above) instead of per-split atomics;
 *   - fp32 weight gradients: slabs in the stream's workspace + a split-ordered reduction, else one split.
 * Audit of the rest: forward contractions (split-K slabs + gemm_finish), attention forward and backward, the norm forwards, the
 * losses (fixed block partials) and sidlsg_adam_ema are order-fixed already; they use no atomics.
 * Guaranteed: equal bits for the same library build, GPU model, shapes, launch configuration and stream assignment.  Not: across
 * builds, batch sizes or split decisions (a different workspace size can change them).  A captured graph keeps the kernels of the
 * mode it was captured in.  on: 1 on, 0 off, -1 query only; returns the previous setting. */
int sidlsg_set_deterministic(int on);

/* ---- normalisation (HBM bound) ------------------------------------------------------------
 * torch.nn.GroupNorm(32, C, eps)+SiLU of ResnetBlock2D.norm1/norm2, Transformer2DModel.norm,
 * conv_norm_out; torch.nn.LayerNorm of BasicTransformerBlock.norm1-3.
 * Mean offsets: the operators are tested (tests/norm_cases.py, profiles/norm_offset_accuracy.txt) with a per-group / per-row
 * |mean| / std of up to 30 at the operator tolerances in fp32 and in bf16, and of up to 100 at 4x those tolerances in fp32.
 * How large the offsets of real SD UNet / VAE activations are has not been measured. */
/* backward: dres (may be NULL, same shape as x) is the gradient reaching x through its other consumer (the residual /
 * shortcut branch of the block that owns the norm); dx = norm-backward + dres in the same pass. */
int sidlsg_groupnorm_ws_floats(int B, int HW, int C, int G); /* host: workspace size in floats, <0 on bad shape */
int sidlsg_groupnorm_nchunks(int B, int HW, int C, int G);   /* host */
int sidlsg_groupnorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* stats, float* ws, int B,
                         int HW, int C, int G, float eps, int silu, void* stream);
int sidlsg_groupnorm_bwd(const void* x, const void* dy, const float* stats, const float* gamma, const float* beta,
                         const void* dres, void* dx, float* dgamma, float* dbeta, float* ws, int B, int HW, int C, int G,
                         int silu, void* stream);
int sidlsg_layernorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* stats, int rows, int C,
                         float eps, void* stream);
int sidlsg_layernorm_bwd_nblocks(int rows); /* host: ws = nblocks*C*2 floats */
/* Deferred dgamma / dbeta reductions (csrc/norm.hip "deferred parameter-gradient reductions"): with deferral on for a stream the norm
 * backward entry points queue their final reduction; sidlsg_flush_reductions launches everything queued for the stream as ONE kernel.
 * The caller keeps every `ws` passed to a deferred call allocated and untouched until the flush.  Return: reductions flushed, < 0 error;
 * sidlsg_pending_reductions: queued reductions, -1 when deferral is off for the stream. */
int sidlsg_defer_reductions(void* stream, int on); /* 1: queue from now on; 2: stop queuing, keep the queue; 0: flush + forget */
int sidlsg_flush_reductions(void* stream);
int sidlsg_pending_reductions(void* stream);
int sidlsg_layernorm_bwd(const void* x, const void* dy, const float* stats, const float* gamma, const void* dres, void* dx,
                         float* dgamma, float* dbeta, float* ws, int rows, int C, void* stream);

/* ---- grouped launches: TWO networks of identical architecture evaluated on ONE stacked batch ---------------------------
 * Phase B of the step evaluates the frozen fake-score network and the frozen teacher on identical inputs
 * (`sid_sd_denoise(unet=fake_score, ...)` and `sid_sd_denoise(unet=true_score, ...)`, sid_training_loop.py:494-506, each a CFG
 * batch through sid_sd_util.py:259-265).  Here both run as ONE pass over a stacked batch [set 0 samples ; set 1 samples]:
 * every weight-bearing kernel takes a second parameter set and picks it per block (rows / samples of the second half), every
 * parameter-free kernel (attention, GEGLU, SiLU, concat) simply sees twice the batch.  One grid of 2x the blocks fills the
 * chip where either network's grid alone does not (16x16 / 8x8 stages, the time-embedding MLP, the 77-token K/V
 * projections), and the frozen passes issue half the launches.  M (rows) resp. B (samples) must be even; the halves need not
 * be tile aligned.  Same epilogue contract as the ungrouped entry points; res / rowvec / outputs are stacked like the input.
 * The backward-data pass of a layer is the same entry point with (dY, transposed weight set 0, transposed weight set 1).
 * bf16 here (the e4m3 forms: "Grouped forms of the e4m3 entry points" below); frozen networks only (there is no grouped weight gradient). */
int sidlsg_gemm_bf16_g2(const void* A, int lda, const void* W, const void* W1, void* C, int ldc, const float* bias, const float* bias1,
                        const void* res, int ldres, const float* rowvec, int ld_rowvec, int rows_per_batch, int M, int N, int K,
                        float alpha, int flags, void* stream);
int sidlsg_conv3x3_bf16_g2(const void* X, int ldx, const void* W, const void* W1, void* Y, int ldc, const float* bias, const float* bias1,
                           const void* res, int ldres, const float* rowvec, int ld_rowvec, int B, int H, int Wd, int Cin, int Cout,
                           int stride, int ups, float alpha, int flags, void* stream);
int sidlsg_groupnorm_fwd_g2(const void* x, const float* gamma, const float* beta, const float* gamma1, const float* beta1, void* y,
                            float* stats, float* ws, int B, int HW, int C, int G, float eps, int silu, void* stream);
int sidlsg_groupnorm_bwd_g2(const void* x, const void* dy, const float* stats, const float* gamma, const float* beta, const float* gamma1,
                            const float* beta1, const void* dres, void* dx, float* ws, int B, int HW, int C, int G, int silu,
                            void* stream);
int sidlsg_layernorm_fwd_g2(const void* x, const float* gamma, const float* beta, const float* gamma1, const float* beta1, void* y,
                            float* stats, int rows, int C, float eps, void* stream);
int sidlsg_layernorm_bwd_g2(const void* x, const void* dy, const float* stats, const float* gamma, const float* gamma1, const void* dres,
                            void* dx, int rows, int C, void* stream);

/* ---- in-library kernel timing (measurement only; bench.py) -------------------------------------------------------------------
 * Kernel durations as `rocprofv3 --kernel-trace` reports them, taken live: while tracing is enabled every `stride`-th CALL of a
 * kernel family launches its kernels with start / stop events bound to the kernel's own dispatch packet (hipExtLaunchKernelGGL) --
 * no extra packets in the stream, unlike events recorded around a launch.  Families: 0 dense GEMM fwd + dgrad, 1 conv3x3 fwd +
 * dgrad, 2 attention forward, 3 attention backward, 4 dense weight gradient, 5 conv weight gradient, 6 GroupNorm forward,
 * 7 GroupNorm backward, 8 LayerNorm forward, 9 LayerNorm backward.  Work = algorithmic flop (0-5) or bytes (6-9) of the call.
 * sidlsg_trace_read (after a device synchronisation; out: 9 doubles, out[7] / out[8] = peak flop/s and bytes/s on input):
 * out[0] summed kernel ms of the sampled calls, out[1] their summed work, out[2] sampled calls, out[3] all calls of the family since
 * enable, out[4] timed kernels, out[5] their summed algorithmic bytes, out[6] their summed roofline time in ms (per call
 * max(flop / peak flop/s, bytes / peak bytes/s): every call is graded against its own bound). */
int sidlsg_trace_enable(int max_kernels);
int sidlsg_trace_pause(int paused);
int sidlsg_trace_set_stride(int family, int stride);
int sidlsg_trace_read(int family, double* out);

/* ---- attention (diffusers Attention + AttnProcessor2_0 / xformers; sid_sd_util.py:102-113) --
 * O = softmax(Q K^T D^-1/2) V per head; Q/K/V/O are strided views ([b][token][h*D + d], token
 * stride ld*, batch stride bs*, in elements) so the fused QKV projection is consumed in place.
 * Admitted head widths: D a multiple of 8 whose round-up to a multiple of 16 is one of 16, 32, 48, 64, 80, 96, 128 or 160, the
 * widths the kernels are tiled for -- D = 8, 16, ..., 96, 120, 128, 152, 160.  Every other D (104, 112, 136 and 144 among them)
 * returns SIDLSG_EINVAL from the forward and the backward, plain and _ps, before anything is launched or written.
 * LSE [B][H][Nq] fp32 (log2 domain) is saved for backward. */
int sidlsg_attn_fwd(const void* Q, const void* K, const void* V, void* O, float* LSE, int B, int H, int Nq, int Nk, int D,
                    int ldq, int ldk, int ldv, int ldo, long long bsq, long long bsk, long long bsv, long long bso,
                    void* stream);
/* backward: dK = dV = NULL -> only dQ (and delta) are produced. */
int sidlsg_attn_bwd(const void* Q, const void* K, const void* V, const void* O, const void* dO, const float* LSE, void* dQ,
                    void* dK, void* dV, float* delta, int B, int H, int Nq, int Nk, int D, int ldq, int ldk, int ldv, int ldo,
                    long long bsq, long long bsk, long long bsv, long long bso, void* stream);
/* The same with PRE-SCALED queries: Q holds q * (D^-1/2 * log2 e) -- the caller folds the factor into the q rows of the
 * projection weight's FORWARD compute copy (sidlsg_scale_cast_ranges: one rounding, like the unscaled copy).  The QK^T
 * accumulators are then seeded with -max / -LSE and feed v_exp_f32 directly.  The backward returns the SAME tensors as
 * sidlsg_attn_bwd: gradients with respect to the unscaled q (= Q / (D^-1/2 log2 e)), k and v -- so the projection's weight
 * gradient is the ordinary one and its backward-data operand is the UNSCALED transposed weight. */
int sidlsg_attn_fwd_ps(const void* Q, const void* K, const void* V, void* O, float* LSE, int B, int H, int Nq, int Nk, int D,
                       int ldq, int ldk, int ldv, int ldo, long long bsq, long long bsk, long long bsv, long long bso,
                       void* stream);
int sidlsg_attn_bwd_ps(const void* Q, const void* K, const void* V, const void* O, const void* dO, const float* LSE, void* dQ,
                       void* dK, void* dV, float* delta, int B, int H, int Nq, int Nk, int D, int ldq, int ldk, int ldv, int ldo,
                       long long bsq, long long bsk, long long bsv, long long bso, void* stream);

/* ---- decoupled cross-attention of an image-prompt adapter (IP-Adapter; csrc/ip_attn.hip), forward only, no LSE -------------------
 * O = softmax(Q K^T D^-1/2) V + s * softmax(Q K2^T D^-1/2) V2 per head, in ONE launch: two key sets (K / V the text, K2 / V2 the image
 * tokens), each softmax normalised on its own, the two results summed in fp32 and rounded once.  Q / O are [B][Nq][ld] views with H
 * heads side by side as in sidlsg_attn_fwd; K, V, K2 and V2 are [B][N*][ld*] views with their own token strides ld* and batch strides
 * bs* (elements): K2 / V2 are typically column slices of one wide per-batch buffer, so ldk2 = ldv2 >> H * D and the pointers carry the
 * column offsets.  s == 0 reads neither K2 nor V2 and gives the one-set attention.
 * Admitted: B, H >= 1; any Nq >= 1; 1 <= Nk <= 128; 1 <= Nk2 <= 32; s finite; bf16 (plain and _ps): D a multiple of 8, 8 <= D <= 160
 * (tiled at D rounded up to 32); fp32: D a multiple of 4, 4 <= D <= 160 (tiled at D rounded up to 16), and the fp32 LDS image
 * 2 * (ceil16(Nk) + ceil16(Nk2)) * (ceil16(D) + 4) * 4 bytes must fit 160 KiB; all six pointers non-null and 16-byte aligned; every
 * ld* >= H * D and every ld*, bs* a multiple of 16 bytes, bs* >= 0; B * H * workgroups-per-head < 2^31.  Anything else returns
 * SIDLSG_EINVAL before anything is launched or written.
 * _ps: Q holds q * (D^-1/2 * log2 e) as for sidlsg_attn_fwd_ps; the one factor serves both sets because they share q.
 * _f32: the fp32 family, nothing rounded to bf16. */
int sidlsg_attn_cross2_fwd(const void* Q, const void* K, const void* V, const void* K2, const void* V2, void* O, float s, int B, int H,
                           int Nq, int Nk, int Nk2, int D, int ldq, int ldk, int ldv, int ldk2, int ldv2, int ldo, long long bsq,
                           long long bsk, long long bsv, long long bsk2, long long bsv2, long long bso, void* stream);
int sidlsg_attn_cross2_fwd_ps(const void* Q, const void* K, const void* V, const void* K2, const void* V2, void* O, float s, int B, int H,
                              int Nq, int Nk, int Nk2, int D, int ldq, int ldk, int ldv, int ldk2, int ldv2, int ldo, long long bsq,
                              long long bsk, long long bsv, long long bsk2, long long bsv2, long long bso, void* stream);
int sidlsg_attn_cross2_fwd_f32(const void* Q, const void* K, const void* V, const void* K2, const void* V2, void* O, float s, int B, int H,
                               int Nq, int Nk, int Nk2, int D, int ldq, int ldk, int ldv, int ldk2, int ldv2, int ldo, long long bsq,
                               long long bsk, long long bsv, long long bsk2, long long bsv2, long long bso, void* stream);

/* Fused backward of the d = 40 self-attention (attn_bwd_fused_kernel: S, dP and the exponentials once for dQ, dK and dV; the key
 * groups' partial dQ go to fp32 slabs in the stream's workspace and are added in a fixed order, so the result is bit-reproducible).
 * Taken inside sidlsg_attn_bwd / _ps when 32 < D <= 48, dK and dV are requested, Nq == Nk is a multiple of 512 and at least the
 * rule's threshold, and one batch element's slabs (H * Nk / 512 * Nq * D * 4 bytes) fit the workspace; every other call keeps the
 * two-kernel path.  A/B switch: environment variable SIDLSG_ATTN_BWD_FUSED (read once) or sidlsg_debug_set_attn_bwd_fused: 0 never,
 * 1 by rule, 2 every call the kernel can run (no length threshold); a negative argument only queries; returns the previous setting.
 * sidlsg_attn_bwd_fused_takes: 1 when a call of that shape (default-stream workspace) takes the fused kernel under the current setting. */
int sidlsg_debug_set_attn_bwd_fused(int mode);
int sidlsg_attn_bwd_fused_takes(int B, int H, int Nq, int Nk, int D, int have_dkdv);

/* ---- scheduler / guidance glue (sid_sd_util.py:182-185, 242, 259-272) ----------------------
 * noisy_input: x_t = s0[b]*x0 + s1[b]*noise (x0 NULL -> zeros: the one-step generator input),
 *   NCHW fp32 in, NHWC bf16 [dup*B][HW][Cp] out (dup=2: [uncond ; cond] halves of the CFG batch),
 *   optional fp32 NCHW copy of x_t.
 * cfg_x0: eps [dup*B][HW][Ce>=C] fp32 -> out NCHW fp32, e = u + kappa*(c-u) when dup=2, by `mode`
 *   (the network's parameterisation):  0 raw: e;  1 x0 from epsilon: (x_t - s1*e)/s0;  2 x0 from v: s0*x_t - s1*e.
 *   Modes 0 and 1 are the former predict_x0 = 0 / 1.  Any other mode -> SIDLSG_EINVAL.
 * cfg_x0_bwd: d_eps NHWC [dup*B][HW][Cp] (zero padded) and, when dxt != NULL, d_xt fp32 NCHW:
 *   mode 0: d_e = g, d_xt = 0;  1: d_e = -s1/s0*g, d_xt = g/s0;  2: d_e = -s1*g, d_xt = s0*g. */
int sidlsg_noisy_input(const float* x0, const float* noise, const float* s0, const float* s1, void* out, float* xt, int B,
                       int C, int HW, int Cp, int dup, void* stream);
int sidlsg_noisy_input_bwd(const void* g, const float* s0, float* dx0, int B, int C, int HW, int Cp, int dup, int accumulate,
                           void* stream);
int sidlsg_cfg_x0(const float* eps, const float* xt, const float* s0, const float* s1, float* out, int B, int C, int HW,
                  int Ce, int dup, float kappa, int mode, void* stream);
int sidlsg_cfg_x0_bwd(const float* g, const float* s0, const float* s1, void* deps, float* dxt, int B, int C, int HW, int Cp,
                      int dup, float kappa, int mode, void* stream);
/* step_renoise: one step boundary of the multi-step generator (sid_sd_util.py:176-185) as one launch.  eps [B][HW][8] fp32 (the
 *   generator's output at t_i), xt fp32 NCHW (x_{t_i}), s0/s1 the coefficients of t_i, s0n/s1n those of t_{i+1}, noise fp32 NCHW
 *   (eps_{i+1}): x_hat = x0 prediction by `mode` (1 epsilon, 2 v; as cfg_x0 with dup = 1), x_{t+1} = s0n*x_hat + s1n*noise ->
 *   out NHWC [B][HW][Cp] activations (channels C.. zero) and xtn fp32 NCHW.  Bit-equal to cfg_x0 followed by noisy_input.
 * step_renoise_bwd: g NHWC [B][HW][Cp] (gradient at the next step's input) and gxtn fp32 NCHW (gradient of x_{t+1}, may be
 *   NULL): d x_hat = s0n*(g + gxtn), then cfg_x0_bwd's formulas: deps NHWC [B][HW][Cp] (zero padded) and, when dxt != NULL,
 *   d x_t fp32 NCHW.  Any other mode -> SIDLSG_EINVAL. */
int sidlsg_step_renoise(const float* eps, const float* xt, const float* s0, const float* s1, const float* s0n, const float* s1n,
                        const float* noise, void* out, float* xtn, int B, int C, int HW, int Cp, int mode, void* stream);
int sidlsg_step_renoise_bwd(const void* g, const float* gxtn, const float* s0, const float* s1, const float* s0n, void* deps,
                            float* dxt, int B, int C, int HW, int Cp, int mode, void* stream);
/* ddim_step: one step boundary of the teacher's deterministic DDIM sampler (Song et al. 2021, eta = 0) as one launch, forward only.
 *   eps [dup*B][HW][Ce>=C] fp32 (the teacher's output at t, halves [uncond ; cond] when dup = 2), xt fp32 NCHW (x_t), s0/s1 [B] the
 *   coefficients sqrt(abar_t) / sqrt(1-abar_t), s0p/s1p [B] those of the previous (smaller) timestep.  All in fp32:
 *   e = u + kappa*(c-u) when dup = 2, else eps (cfg_x0 mode 0);  x0 by `mode` (1 epsilon, 2 v) as cfg_x0;  eps_hat = e (mode 1) or
 *   s0*e + s1*x_t (mode 2);  x_prev = s0p*x0 + s1p*eps_hat (noisy_input's expression) -> out NHWC [dup*B][HW][Cp] activations (both
 *   halves equal, channels C.. zero; NULL on the last step), xtn fp32 NCHW, x0 fp32 NCHW (may be NULL).  In mode 1 the three outputs
 *   are bit-equal to cfg_x0(mode 1), cfg_x0(mode 0), noisy_input(x0, e, s0p, s1p, dup); in mode 2 x0 is bit-equal to cfg_x0(mode 2).
 *   dup other than 1 / 2, mode other than 1 / 2, a NULL eps / xt / coefficient / xtn -> SIDLSG_EINVAL, nothing launched. */
int sidlsg_ddim_step(const float* eps, const float* xt, const float* s0, const float* s1, const float* s0p, const float* s1p,
                     void* out, float* xtn, float* x0, int B, int C, int HW, int Ce, int Cp, int dup, float kappa, int mode,
                     void* stream);
/* solver_step (csrc/solver.hip): one step boundary of the teacher's solver family (DDIM with any eta, DPM-Solver++ 2M) as one launch,
 * forward only.  eps / xt / s0 / s1 / dup / kappa / mode / Ce / Cp as ddim_step; coef [B][4] = (c_x, c_cur, c_prev, c_n) of
 * scheduler.solver_schedule; x0p fp32 NCHW the x0 prediction of the step before (may be NULL); noise fp32 NCHW (may be NULL); scale
 * [B] the guidance-rescale factors of cfg_rescale_stats (may be NULL).  All in fp32:
 *   e = u + kappa*(c-u) when dup = 2, else eps;  e = e*scale[b] when scale is given;  x0 by `mode` as cfg_x0 (bit-equal to it when
 *   scale is NULL);  x_t = c_x*x_s + c_cur*x0 + c_prev*x0p + c_n*noise: one rounded product, then one fma per term in this order; a
 *   NULL x0p / noise term is not formed (the bits of a zero tensor with a zero coefficient)
 *   -> out NHWC [dup*B][HW][Cp] activations (both halves equal, channels C.. zero; NULL on the last step), xtn fp32 NCHW, x0 fp32
 *   NCHW (may be NULL; the next step's x0p).
 * The coefficients live on the device, so the caller says whether this step's c_prev is non-zero: need_prev != 0 with a NULL x0p,
 * dup other than 1 / 2, mode other than 1 / 2, a NULL eps / xt / s0 / s1 / coef / xtn -> SIDLSG_EINVAL, nothing launched. */
int sidlsg_solver_step(const float* eps, const float* xt, const float* s0, const float* s1, const float* coef, const float* x0p,
                       const float* noise, const float* scale, void* out, float* xtn, float* x0, int B, int C, int HW, int Ce, int Cp,
                       int dup, float kappa, int mode, int need_prev, void* stream);
/* cfg_rescale_stats: scale[b] = phi*std(c_b)/std(g_b) + 1 - phi, g = u + kappa*(c-u), for eps [2*B][HW][Ce>=C] fp32 ([uncond ; cond]):
 * the guidance rescale of Lin et al. 2024 (diffusers' rescale_noise_cfg) as one factor per sample.  Unbiased standard deviations over
 * the C*HW real channels, centred (two passes), summed in a fixed order without atomics; std(g_b) = 0 gives the factor 1 (diffusers
 * yields NaN).  C*HW < 2 or a NULL pointer -> SIDLSG_EINVAL. */
int sidlsg_cfg_rescale_stats(const float* eps, float* scale, int B, int C, int HW, int Ce, float kappa, float phi, void* stream);
/* masked_renoise (csrc/inpaint.hip): the masked step boundary of inpainting as one launch, forward only.  x fp32 NCHW [B][C][HW] is
 * what a sampler step produced at its target level, z0 fp32 NCHW the scaled init latents, noise fp32 NCHW the initial noise (may be
 * NULL), mask uint8 [B][HW], or [1][HW] when mask_shared != 0 (nonzero: repaint), a0 / a1 [B] the coefficients of the target level
 * (a0 NULL means 1; a1 is given exactly when noise is):
 *   known = a0*z0 + a1*noise: rounded a1*noise, then one fma -- bit-equal to the fp32 x_t of noisy_input(z0, noise, a0, a1); without
 *   noise known = a0*z0 (one rounded product), without noise and a0 it is z0 itself;  xn = mask ? x : known, a select
 *   -> xn fp32 NCHW (may be x itself) and, when out != NULL, the next network input NHWC [dup*B][HW][Cp] activations (both halves
 *   equal, channels C.. zero), bit-equal to noisy_input(NULL, xn, 1, 1, dup).
 * A NULL x / z0 / mask / xn, C > 8, Cp % 8 or Cp < 8, dup other than 1 / 2, noise without a1 or a1 without noise, B*HW > 2^31 - 1
 * -> SIDLSG_EINVAL, nothing launched. */
int sidlsg_masked_renoise(const float* x, const float* z0, const float* noise, const unsigned char* mask, const float* a0,
                          const float* a1, void* out, float* xn, int B, int C, int HW, int Cp, int dup, int mask_shared, void* stream);

/* ---- losses with closed-form gradients (sid_training_loop.py:423-445, 508-530) -------------
 * Per-sample NaN filtering is done in-kernel (a sample containing NaN contributes 0 and gets zero
 * gradients), `scale` = loss_scaling / batch_gpu_total.  ws >= 2*S + 8*S floats.  loss: 1 float.
 * S <= 0 or n <= 0: SIDLSG_EINVAL. */
int sidlsg_g_loss(const float* x, const float* yr, const float* yf, float* dx, float* dyr, float* dyf, float* loss, float* ws,
                  int S, int n, float alpha, float scale, void* stream);
int sidlsg_fake_loss(const float* e, const float* noise, float* de, float* loss, float* ws, int S, int n, float scale,
                     void* stream);
/* v-prediction fake-score loss (sid_training_loop.py:423-445, v branch) of a network output o against the velocity target
 * v* = s0[s]*noise - s1[s]*x0, formed in-kernel (never written).  o, x0 (the generator's images), noise: [S][n] fp32;
 * s0, s1, w: [S] fp32 in device memory (w = snr/(snr+1), snr = abar/(1-abar): DDPMScheduler.snr_weights).
 * loss[0] = scale * sum_s w[s] * sum_i (o - v*)^2 over the samples whose o and v* hold no NaN; de = 2*scale*w[s]*(o - v*),
 * zero for a dropped sample.  Same two-stage reduction and workspace as sidlsg_fake_loss: ws >= 2*S + 8*S floats. */
int sidlsg_fake_loss_v(const float* o, const float* x0, const float* noise, const float* s0, const float* s1, const float* w,
                       float* de, float* loss, float* ws, int S, int n, float scale, void* stream);

/* ---- optimizer: nan_to_num + clip + Adam/AdamW + EMA + bf16 weight copy + zero_grad --------
 * (sid_training_loop.py:458-462, 541-565; sid_train.py:219-226).  hyper: 13 floats in DEVICE memory:
 * lr, beta1, beta2, eps, bias_corr1, sqrt(bias_corr2), ema_beta, weight_decay, decoupled, clip, grad_scale, 1 - beta1, 1 - beta2
 * (the last two rounded from double, as torch forms the weights of lerp_ and addcmul_).
 * m may be NULL when beta1 == 0; ema, w_bf16 may be NULL. */
int sidlsg_adam_ema(float* p, float* g, float* m, float* v, float* ema, void* w_bf16, const float* hyper, long long n,
                    int zero_grad, void* stream);

/* ---- small elementwise / layout kernels ---------------------------------------------------- */
int sidlsg_timestep_embed(const long long* t, void* out, int B, int dim, void* stream); /* Timesteps(flip_sin_to_cos) */
int sidlsg_silu_fwd(const void* x, void* y, long long n, void* stream);
int sidlsg_silu_bwd(const void* x, const void* dy, void* dx, long long n, void* stream);
int sidlsg_geglu_fwd(const void* h, void* y, long long M, int F, void* stream);           /* diffusers GEGLU */
int sidlsg_geglu_bwd(const void* h, const void* dy, void* dh, long long M, int F, void* stream);
int sidlsg_concat2(void* a, void* b, void* out, long long M, int C1, int C2, int to_parts, void* stream); /* skip concat */
int sidlsg_sumpool2x2(const void* g, void* out, int B, int H, int W, int C, void* stream);   /* bwd of nearest x2 */
int sidlsg_zero_insert2(const void* g, void* out, int B, int Ho, int Wo, int H, int W, int C, void* stream); /* bwd-data of stride 2: out [B][H][W][C] */
int sidlsg_add_bf16(const void* a, const void* b, void* o, long long n, void* stream);
int sidlsg_colsum_nchunks(int B, int rows_per_batch); /* host: grid.x of the reduction */
int sidlsg_colsum(const void* g, int ldg, float* per_batch, float* total, float* ws, int B, int rows_per_batch, int N,
                  void* stream); /* bias / time-embedding gradients: per_batch[B][N] += (zero it first), total[N] +=; ws unused */
/* the same with a row stride for per_batch (elements, >= N): the 22 ResBlocks of a pass accumulate their time-embedding column
 * gradients straight into their column slices of ONE [B][sum Cout] buffer (one fill per pass instead of 22, no concat kernel) */
int sidlsg_colsum_strided(const void* g, int ldg, float* per_batch, int ld_pb, float* total, int B, int rows_per_batch, int N, void* stream);
int sidlsg_cast_f32_bf16(const float* x, void* y, long long n, void* stream);
int sidlsg_cast_bf16_f32(const void* x, float* y, long long n, void* stream);
int sidlsg_transpose_w(const float* src, void* dst, int N, int K, int T, void* stream); /* [N][T][K] -> [K][T rev][N] bf16 */
/* All backward-data operands of a network in ONE launch.  jobs: DEVICE array of njobs records
 *   struct sidlsg_tw_job { const float* src; void* dst; int N, K, T, blk0; };   (32 bytes, no padding)
 * sorted by blk0 = index of the job's first 32x32 tile (job i covers T*ceil(N/32)*ceil(K/32) tiles); nblocks = total. */
int sidlsg_transpose_w_batched(const void* jobs, int njobs, int nblocks, void* stream);
/* Same, from the bf16 COMPUTE copies (src of a record points at bf16 [N][T][K]; 4 instead of 6 bytes per parameter):
 * 64x64 tiles -> blk0 / nblocks count ceil(N/64)*ceil(K/64) tiles per tap; N and K multiples of 8. */
int sidlsg_transpose_w16_batched(const void* jobs, int njobs, int nblocks, void* stream);
/* Scaled re-cast of parameter ranges, dst[i] = bf16(scale * src[i]): folds the attention's D^-1/2 log2(e) factor into the q
 * rows of a projection weight's bf16 COMPUTE copy (sidlsg_attn_fwd_ps).  jobs: DEVICE array of
 *   struct { const float* src; void* dst; int n, blk0; float scale; int pad; }   (32 bytes)
 * sorted by blk0 = index of the job's first block of 2048 elements; nblocks = total. */
int sidlsg_scale_cast_ranges(const void* jobs, int njobs, int nblocks, void* stream);

/* ---- LoRA merge (csrc/lora.hip): low-rank updates of fp32 master weights, every touched layer of a network in ONE launch ------
 * Replaces the per-layer `W += scale * alpha / rank * (up @ down)` of the kohya / diffusers loaders.  For every job
 *   dst[n][k] = base[n][k] + sum_r coef[r] * up[n][r] * down[r][k],   n < N, k < KK, r < R, everything fp32,
 * on v_mfma_f32_16x16x4_f32: c = coef[r] * up[n][r] is rounded once, the sum is an fp32 fma chain over r in ascending order starting
 * from 0, and base is added once at the end.  No atomics; every element of dst is written exactly once, by the lane that read the
 * same element of base, so base == dst (in place) is allowed and two launches on the same inputs give the same bits.  No other
 * overlap between a job's dst and any operand of the launch is allowed.
 * KK is the physical row of a master: Cin of a Linear / 1x1 conv, 9 Cin of a 3x3 conv in the [Cout][3][3][Cin] layout (the caller
 * permutes `down` to that order).  coef[r] carries scale * alpha / rank of the adapter that column r belongs to; adapters on one
 * layer are concatenated along R.
 * jobs: DEVICE array, jobs_host: a HOST copy of the same njobs records (read only during the call).  Only the host copy can be
 * validated before the launch and only the device copy is read by the kernel: the CALLER guarantees that the two are byte-identical
 * and that the device copy is not modified before the launch has run.  A device copy that differs is an unvalidated launch.
 *   struct sidlsg_lora_job { const float* base; float* dst; const float* up; const float* down; const float* coef;
 *                            int N, KK, R, blk0; };                                             (56 bytes, no padding)
 * base, dst [N][KK]; up [N][R]; down [R][KK]; coef [R].  Sorted by blk0 = index of the job's first 64 x 64 output tile, gap-free
 * from 0: job i covers ceil(N/64) * ceil(KK/64) tiles; nblocks = their total.
 * Admitted: all five pointers 16-byte aligned; N >= 1; KK % 4 == 0; R % 4 == 0, 4 <= R <= 4096 (pad with zero-coef columns);
 * N * KK * 4 < 2^31 per job.  Anything else, a blk0 out of sequence or an nblocks that is not the total: SIDLSG_EINVAL, nothing
 * is launched.  Edges of N and KK are predicated, nothing around a job's ranges is read or written. */
int sidlsg_lora_merge_f32(const void* jobs_host, const void* jobs, int njobs, int nblocks, void* stream);

/* ---- precision / recall (metrics/sid_precision_recall.py): fp16 feature distances on the MFMA, reduced in registers ----------
 * Feature matrices are [n][F] fp16 row-major, F a positive multiple of 32 (pad with zero columns on the host), 16-byte aligned.
 * In all three, exactly:  d2(i, j) = max(|a_i|^2 + |b_j|^2 - 2 a_i . b_j, 0)  with a . b on v_mfma_f32_16x16x32_f16 (fp32
 * accumulate) and the norms in fp32;  d(i, j) = fp16_rne(sqrt(d2)).  The three share one tile routine, so a distance has the same
 * bits whichever entry forms it.
 * sidlsg_pr_distances: out[R][C] fp16 = d(rows_i, cols_j), the dense form (compute_distances, :19-32).
 * sidlsg_pr_kth_radius: radius_out[N] fp16 = the (k+1)-th smallest d over ALL N columns of the set against itself, the row
 *   itself included and equal values counted as often as they occur (`dist.kthvalue(nhood_size + 1)`, :59); 0 <= k <= 7,
 *   N >= k + 1.  No [N][N] buffer.
 * sidlsg_pr_member: inside_out[P] bytes, 1 where some column j has d(probe_i, manifold_j) <= radius[j] (:64), else 0.
 * SIDLSG_EINVAL, and no launch, for null or misaligned pointers, F % 32 != 0, k > 7 or N < k + 1. */
int sidlsg_pr_distances(const void* rows, int R, const void* cols, int C, int F, void* out, void* stream);
int sidlsg_pr_kth_radius(const void* manifold, int N, int F, int k, void* radius_out, void* stream);
int sidlsg_pr_member(const void* probes, int P, const void* manifold, int N, int F, const void* radius, void* inside_out, void* stream);

/* ---- KID / CMMD (kernel two-sample statistics): fp32 Gram tiles on the f32 MFMA, kernel values summed in fp64 ------------------
 * X, Y: [n][F] fp32 row-major, F a positive multiple of 4 (pad with zero columns on the host), 16-byte aligned.  Subset s uses the
 * rows X[ix[s][i]], i < mx, and Y[iy[s][j]], j < my (ix: int32 [S][mx], iy: [S][my], indices trusted to be in range); both lists
 * NULL = the rows 0..n-1 in order, then S = 1, mx = nx, my = ny.  No gathered copy and no N x N matrix is formed.
 * out[s] = {Sxx, Syy, Sxy, Txx, Tyy} (doubles): S** = the sum of v over ALL ordered pairs of the two row lists, the diagonal
 * included; T** = the sum over i == j of the symmetric passes.  With g = a . b on v_mfma_f32_16x16x4_f32 (an exact fp32 fma chain
 * over k, in the same order for every pair and for the norms), in fp32:
 *   kind 0 (polynomial):  v = t * t * t,  t = fma(p0, g, p1)
 *   kind 1 (RBF):         d2 = max(fma(-2, g, |a|^2 + |b|^2), 0),  v = -expm1f(-(p0 * d2))  = 1 - exp(-p0 d2), the COMPLEMENT of the
 *                         kernel value (full relative precision where the kernel is close to 1).  A row against itself or a
 *                         bit-identical duplicate gives d2 = 0 and v = 0 exactly.
 * Each v is converted to double; one double per 128 x 128 tile and quantity goes to ws, and a second launch adds the slots of a
 * subset in a fixed order: no atomics, the same inputs give the same bits on every run.  ws: sidlsg_pair_kernel_sums_ws_doubles(S,
 * mx, my) doubles (a host query; negative for sizes the entry point rejects).
 * SIDLSG_EINVAL, and no launch, for null or misaligned pointers, F % 4 != 0, S < 1 or > 65535, mx or my < 1, n, mx or my > 2^24,
 * F > 2^20, an index list on one side only, no lists with S != 1 or m != n, kind outside {0, 1}, or a workspace of 2^31 doubles or more. */
int sidlsg_pair_kernel_sums_ws_doubles(int S, int mx, int my);
int sidlsg_pair_kernel_sums(const float* X, int nx, const float* Y, int ny, int F, const int* ix, const int* iy, int S, int mx, int my,
                            int kind, float p0, float p1, double* out, double* ws, void* stream);

/* ---- FID Inception-v3 detector (sid_lsg_amd/inception.py, csrc/inception.hip): fp32 only ------------------------------------------
 * sidlsg_conv2d_relu_f32: Y[b][ho][wo][n] = act(bias[n] + sum over (dh, dw, c) of X[b][ho * stride - pad_h + dh][wo * stride - pad_w + dw][c]
 * * W[n][dh][dw][c]) on v_mfma_f32_16x16x4_f32: an exact fp32 fma chain in increasing k = (dh * KW + dw) * Cin + c, then one add of the
 * bias (the folded BatchNorm shift; never NULL), then max(., 0) when relu != 0.  X: [B][H][Wd][ldx] NHWC, W: [Cout][KH][KW][Cin],
 * Y: [B][Ho][Wo][ldc] with Ho = (H + 2 pad_h - KH) / stride + 1 (floor), Wo likewise.  ldc is independent of Cout: Y may point at a
 * channel slice of a wider buffer, the columns outside [0, Cout) of a row are not touched.  Taps outside the image read as zero (a
 * bounds test in the gather, no padded copy).  (KH, KW) in {(1,1), (3,3), (5,5), (1,7), (7,1), (1,3), (3,1)}, stride 1 or 2,
 * 0 <= pad < kernel side, Cin, ldx, ldc multiples of 4 (a 3-channel image is fed as 4 channels with a zero plane and zero weights),
 * any Cout and any B * Ho * Wo.  All four pointers 16-byte aligned.
 * sidlsg_pool2d_f32: k x k window (k <= 8, 2 pad <= k) over X [B][H][W][ldx] -> Y [B][Ho][Wo][ldy], C channels (C, ldx, ldy multiples
 * of 4).  mode 0: max over the taps inside the image (padding never wins: the bits of max_pool2d).  mode 1: mean over the taps inside
 * the image only (count_include_pad = False): summed in row-major order, divided once by their count.
 * sidlsg_inception_input_u8: uint8 NCHW [B][3][H][W] -> out [B][299][299][4] fp32, TF's legacy bilinear resize and the detector's
 * normalisation in one launch.  Output column i reads q = (i * W) div 299 and min(q + 1, W - 1) with the weight
 * float((i * W) mod 299) / 299.0f on the second (rows likewise); t = a + l * (b - a) horizontally, then vertically, then
 * (t - 128) / 128, each operation rounded once; channel 3 is zero.  H, W <= 16384.
 * SIDLSG_EINVAL, and no launch, for anything outside this and for an operand of 2^31 bytes or more. */
int sidlsg_conv2d_relu_f32(const float* X, int ldx, const float* W, float* Y, int ldc, const float* bias, int B, int H, int Wd, int Cin,
                           int Cout, int KH, int KW, int stride, int pad_h, int pad_w, int relu, void* stream);
int sidlsg_pool2d_f32(const float* X, int ldx, float* Y, int ldy, int B, int H, int W, int C, int k, int stride, int pad, int mode,
                      void* stream);
int sidlsg_inception_input_u8(const void* images, float* out, int B, int H, int W, void* stream);

/* ---- paired image fidelity: PSNR, SSIM, LPIPS (sid_lsg_amd/fidelity.py, csrc/fidelity.hip) ----------------------------------------
 * No atomics, no data-dependent loops: one workspace slot per workgroup and quantity, added by a second launch in a fixed order, so
 * the same inputs give the same bits on every run.
 * sidlsg_psnr_ssim_u8: a, b uint8 [B][3][H][W]; mask uint8 [B][H][W] or NULL (NULL = every pixel kept); a pixel is KEPT when its
 *   mask byte is < 128 (the convention of --mask_images).  out [B][8] doubles:
 *     0 sse       sum over the 3 channels and all pixels of (a - b)^2 (an integer below 2^53, exact in the double)
 *     1 n         number of terms of sse = 3 H W
 *     2 ssim_sum  sum of the SSIM index over the 3 channels and the (H - 10) x (W - 10) valid window centres
 *     3 ssim_n    number of terms of ssim_sum
 *     4..7        the same four restricted to kept positions; a kept SSIM term is a window whose CENTRE pixel is kept (the window
 *                 itself may cover pixels that are not).
 *   SSIM (Wang et al.): 11 x 11 separable Gaussian window, sigma 1.5, weights exp(-x^2 / (2 sigma^2)), x = -5..5, normalised (built
 *   in double on the host); K1 = 0.01, K2 = 0.03, L = 255; population moments; valid windows only.  The five window moments
 *   (x, y, x^2, y^2, xy: the horizontal pass first, then the vertical) and the formula
 *   ((2 mx my + C1)(2 cov + C2)) / ((mx^2 + my^2 + C1)(vx + vy + C2)) are evaluated in fp64, each operation rounded once; a window
 *   over bit-identical pixels gives exactly 1.  ws: sidlsg_psnr_ssim_ws_doubles(B, H, W) doubles (a host query; negative for
 *   sizes the entry point rejects).  SIDLSG_EINVAL, and no launch, for H or W < 11, B < 1 or > 21845, null a / b / out / ws, out or
 *   ws not 8-byte aligned, an operand of 2^31 bytes or more.
 * sidlsg_lpips_input_u8: a, b uint8 [B][3][H][W] -> out fp32 NHWC [2B][H][W][4], rows 0..B-1 from a, rows B..2B-1 from b, channel 3
 *   zero (the 4-channel feed of sidlsg_conv2d_relu_f32).  In fp32, exactly: t = x / 127.5f; t = t - 1; (t - shift_c) / scale_c, IEEE
 *   divisions.  out 16-byte aligned, scale_c != 0, fewer than 2^31 output bytes; SIDLSG_EINVAL and no launch otherwise.
 * sidlsg_lpips_layer_f32: F fp32 NHWC [2B][h][wd][ldf] of which the first C channels are read, w [C] ->
 *   out[i] (double) = mean over the h wd pixels of  sum_c w_c (f0_c / (|f0|_2 + 1e-10) - f1_c / (|f1|_2 + 1e-10))^2,  f0 the pixel of
 *   row i, f1 that of row B + i, the norms over the C channels.  Per pixel in fp32, each operation rounded once: 16 lanes share a
 *   pixel, lane l sums the elements of its 16-byte chunks l, l + 16, .. in channel order, the lanes are added by an xor butterfly
 *   (8, 4, 2, 1); the pixel values are added in double.  Bit-identical f0 and f1, and a pixel that is all zero in both, give exactly
 *   0.  ws: sidlsg_lpips_layer_ws_doubles(B, h, wd) doubles.  C and ldf multiples of 4, ldf >= C, F and w 16-byte aligned, out and
 *   ws 8-byte aligned, B <= 32767, F below 2^31 bytes; SIDLSG_EINVAL and no launch otherwise.
 * sidlsg_lpips_sum_f64: vals [taps][B] doubles -> out[i] = ((vals[0][i] + vals[1][i]) + vals[2][i]) + .., the taps of a pair added in
 *   order: a pair's LPIPS does not depend on the batch it travels in (a library reduction may pick its order by the shape).
 *   1 <= taps <= 64, 1 <= B <= 32767, 8-byte aligned pointers; SIDLSG_EINVAL and no launch otherwise.
 * sidlsg_lpips_group_f32: the all-pairs form of sidlsg_lpips_layer_f32.  F fp32 NHWC [G*K][h][wd][ldf], group g = rows gK .. gK+K-1;
 *   out [G][P] doubles, P = K (K - 1) / 2, pairs (i, j), i < j, in lexicographic order: (0,1), (0,2), .., (0,K-1), (1,2), ..
 *   out[g][p(i,j)] has exactly the bits sidlsg_lpips_layer_f32 writes for the pair (row gK+i, row gK+j): the same per-lane channel
 *   order, butterfly, norm, division, difference, weighted square, per-group double sums in pixel order, one slot per 128-pixel
 *   block and the same final reduction.  Maps of 512 pixel blocks and more (over all groups) are read once, every vector normalised
 *   once and all pairs formed on chip; smaller ones, and groups too large for LDS, spread the pairs over the grid (see
 *   sidlsg_lpips_group_form_f32).  A pair's value
 *   does not depend on G, on K or on where the pair sits; an identical pair gives exactly 0, an all-zero pixel contributes 0.  No
 *   atomics.  ws: sidlsg_lpips_group_ws_doubles(G, K, h, wd) doubles (negative outside the admitted set).  2 <= K <= 16, G >= 1,
 *   G K <= 32767, G P <= 32767, C >= 4, C and ldf multiples of 4, ldf >= C, F and w 16-byte aligned, out and ws 8-byte aligned, F
 *   below 2^31 bytes, G P ceil(h wd / 128) below 2^31; SIDLSG_EINVAL, no launch and out untouched otherwise.
 * sidlsg_lpips_group_form_f32: the same with the launch form named: 1 = one workgroup per 128-pixel block and group, all pairs formed
 *   on chip (one read of F); it keeps the K normalised vectors of 128 pixels in LDS and is SIDLSG_EINVAL where they do not fit in
 *   64 KB next to the 128 P bytes of accumulators (2048 K ceil(C / 64) bytes: C 128 from K 14, C 256 from K 8, C 512 from K 4).
 *   2 = one workgroup per block, pair and group (the paired kernel's grid without the gathered copies; every map is read K - 1
 *   times).  0 = form 1 where it is admitted and has at least 512 workgroups, else form 2, which is what sidlsg_lpips_group_f32
 *   does.  The forms write the same bits; the tests and tools/fidelity_cost.py name them.  Any other form is SIDLSG_EINVAL. */
int sidlsg_psnr_ssim_ws_doubles(int B, int H, int W);
int sidlsg_psnr_ssim_u8(const void* a, const void* b, const void* mask, int B, int H, int W, double* out, double* ws, void* stream);
int sidlsg_lpips_input_u8(const void* a, const void* b, float* out, int B, int H, int W, float shift0, float shift1, float shift2,
                          float scale0, float scale1, float scale2, void* stream);
int sidlsg_lpips_layer_ws_doubles(int B, int h, int wd);
int sidlsg_lpips_layer_f32(const float* F, int ldf, const float* w, int B, int h, int wd, int C, double* out, double* ws, void* stream);
int sidlsg_lpips_sum_f64(const double* vals, int taps, int B, double* out, void* stream);
int sidlsg_lpips_group_ws_doubles(int G, int K, int h, int wd);
int sidlsg_lpips_group_f32(const float* F, int ldf, const float* w, int G, int K, int h, int wd, int C, double* out, double* ws, void* stream);
int sidlsg_lpips_group_form_f32(const float* F, int ldf, const float* w, int G, int K, int h, int wd, int C, int form, double* out, double* ws,
                                void* stream);

/* ---- snapshot preview grids (save_image_grid, sid_training_loop.py:99-115, 597-614) -------------------------------------
 * B decoded fp32 images -> their tiles of ONE uint8 grid image [gh*H][gw*W][3] (HWC, what a PNG writer takes): image i goes to
 * tile first + i, row (first + i) / gw, column (first + i) % gw, so the batches of a grid are placed as they leave the decoder and
 * the fp32 images are never concatenated, permuted or copied to the host.  layout 0: src [B][H][W][8] (NHWC, channels 3..7 are
 * padding: the VAE decoder's native output); layout 1: src [B][3][H][W].  In fp32, exactly: v = (x - lo) * scale (two roundings,
 * scale = 255 / (hi - lo) formed in double on the host and rounded once: 127.5 for [-1, 1], 1 for [0, 255]), round to nearest
 * even, clamp to [0, 255]; NaN -> 0 (numpy leaves that cast undefined).  W % 4 == 0, src 16-byte aligned.  SIDLSG_EINVAL, and no
 * launch, for first + B > gw*gh, hi == lo, null pointers or a grid of 2 GiB or more. */
int sidlsg_image_grid_u8(const float* src, void* grid, int B, int H, int W, int layout, int first, int gw, int gh, float lo, float hi,
                         void* stream);

/* ---- CLIP image tower (networks/clip.py; the ViT itself runs on the GEMM / LayerNorm / attention entry points above) ----------
 * sidlsg_clip_patches_u8(_f32): the wrapper's preprocessing (networks/clip.py:33-37) in one launch.  images: uint8 [B][3][H][W]
 *   (H and W may differ).  In fp32, exactly: v = x / 255; bicubic resampling to R x R with F.interpolate(mode='bicubic',
 *   align_corners=False) semantics (A = -0.75, source coordinate (dst + 0.5) * in / out - 0.5, tap indices clamped to the border, no
 *   antialiasing, overshoot not clamped); (v - mean_c) / std_c.  out: bf16 (_f32: fp32) [B * (1 + (R/P)^2)][Kp], the A operand of
 *   the patch-embedding GEMM: one row per token slot, column (c * P + py) * P + px (the flattened patch_embedding.weight); columns
 *   3*P*P .. Kp - 1 and the whole class-token row (row 0 of every image) are written as zeros, so ONE GEMM whose res operand holds
 *   the position embeddings (class embedding added into row 0) yields the token tensor.  R % P == 0, Kp % 8 == 0, Kp >= 3*P*P, out
 *   16-byte aligned, std != 0, fewer than 2^31 input bytes and output elements; SIDLSG_EINVAL and no launch otherwise.
 * sidlsg_gelu(_f32): y = act(x) on n bf16 (fp32) elements, evaluated in fp32.  mode 0: quick_gelu x * sigmoid(1.702 x) (OpenAI
 *   checkpoints); mode 1: the exact GELU x * Phi(x) (open_clip ViT-H / ViT-g), as 0.5 x erfc(-x / sqrt 2).  x, y 16-byte aligned; any n.
 * sidlsg_clip_score: img, txt [B][F] bf16 (f32_in != 0: fp32) -> feats [B][2F] fp32 = F.normalize(img) | F.normalize(txt) (x /
 *   max(|x|_2, 1e-12): the wrapper's return value, :39-53) and cosine [B] fp32, the dot product of the two halves.  One wave per
 *   row, fp32 accumulation. */
int sidlsg_clip_patches_u8(const void* images, void* out, int B, int H, int W, int R, int P, int Kp, float mean0, float mean1, float mean2,
                           float std0, float std1, float std2, void* stream);
int sidlsg_clip_patches_u8_f32(const void* images, void* out, int B, int H, int W, int R, int P, int Kp, float mean0, float mean1,
                               float mean2, float std0, float std1, float std2, void* stream);
int sidlsg_gelu(const void* x, void* y, long long n, int mode, void* stream);
int sidlsg_gelu_f32(const void* x, void* y, long long n, int mode, void* stream);
int sidlsg_clip_score(const void* img, const void* txt, int f32_in, float* feats, float* cosine, int B, int F, void* stream);

/* ---- AutoencoderKL.encode (sid_lsg_amd/vae.py HipAutoencoderKLEncoder; the reference never encodes images: no counterpart there) ----
 * sidlsg_conv3x3_br_bf16: diffusers Downsample2D(padding = 0): F.pad(x, (0, 1, 0, 1)) + conv2d(k = 3, stride 2, padding 0), i.e.
 *   Y(i, j) = sum_{u, v} W(u, v) X(2 i + u, 2 j + v) with X = 0 at row H and column Wd.  X: [B][H][Wd][ldx] bf16, W: [Cout][3][3][Cin],
 *   Y: [B][H/2][Wd/2][ldc] bf16 (fp32 with SIDLSG_OUT_F32); epilogue: bias (may be NULL), SIDLSG_SILU.  Forward only.  H and Wd even,
 *   Cin and ldx multiples of 8; SIDLSG_EINVAL otherwise.  sidlsg_conv3x3_bf16 and its dispatch are untouched by it.
 * sidlsg_attn_fwd_wide: O = softmax(Q K^T D^-1/2) V for ONE head of width D = 512 (any other D: SIDLSG_EINVAL), forward only: bf16 in and
 *   out, fp32 accumulation, online softmax over 32-key tiles, no N x N matrix in memory.  Q/K/V/O: [B][N][ld*] views (token stride ld*,
 *   batch stride bs*, in elements, multiples of 8; Q/K/V 16-byte aligned), N a multiple of 16 (queries = keys).
 * sidlsg_image_to_nhwc8(_f32): images -> the [B][H][W][8] bf16 activation conv_in takes (channels 3..7 zero).  uint8 [B][H][W][3]:
 *   x / 127.5 - 1 in fp32 (IEEE division, then subtraction), rounded to nearest even; _f32: fp32 [B][3][H][W] already in [-1, 1], rounded.
 * sidlsg_vae_posterior: the tail of encode in one launch.  moments [B][HW][8] fp32 (conv_out, NHWC) -> quant_conv (qw [8][8], qb [8]
 *   fp32: out = qw moments + qb per pixel) -> mean | logvar = channels 0..3 | 4..7, logvar clamped to [-30, 20], std = exp(logvar / 2),
 *   z = (mean + std * eps) * scaling, or mean * scaling when eps = NULL (the mode).  eps, z, and (when not NULL) mean, logvar
 *   (clamped): fp32 NCHW [B][4][HW]. */
int sidlsg_conv3x3_br_bf16(const void* X, int ldx, const void* W, void* Y, int ldc, const float* bias, int B, int H, int Wd, int Cin, int Cout,
                           int flags, void* stream);
int sidlsg_attn_fwd_wide(const void* Q, const void* K, const void* V, void* O, int B, int N, int D, int ldq, int ldk, int ldv, int ldo,
                         long long bsq, long long bsk, long long bsv, long long bso, void* stream);
int sidlsg_image_to_nhwc8(const void* images_u8, void* out, int B, int H, int W, void* stream);
int sidlsg_image_to_nhwc8_f32(const float* images_nchw, void* out, int B, int H, int W, void* stream);
int sidlsg_vae_posterior(const float* moments, const float* qw, const float* qb, const float* eps, float* z, float* mean, float* logvar, int B,
                         int HW, float scaling, void* stream);

/* ---- ControlNet (sid_lsg_amd/controlnet.py HipControlNet; the reference has no structure conditioning: no counterpart there) ----------
 * sidlsg_control_hint_u8: control images uint8 [B][H][W][3] (RGB) -> the hint embedder's input [B][H][W][8], bf16 (f32_out != 0: fp32),
 *   float(x) / 255 as one IEEE fp32 division, for bf16 rounded to nearest even; channels 3..7 zero.  out 16-byte aligned and below
 *   2^31 bytes; SIDLSG_EINVAL and no launch otherwise.  Every contraction of a ControlNet runs on the GEMM / conv entry points above. */
int sidlsg_control_hint_u8(const void* images_u8, void* out, int B, int H, int W, int f32_out, void* stream);

/* ---- Canny control maps and edge adherence (sid_lsg_amd/edges.py, csrc/canny.hip; the reference has no counterpart) -----------------
 * Integer arithmetic throughout: every result is specified to the bit.  The rules restate OpenCV's Canny(img, low, high, apertureSize
 * = 3, L2gradient = false) on a 3-channel 8-bit image, which with (100, 200) is ControlNet's Canny annotator.
 * EDGE MAPS travel as BIT PLANES: uint32 [B][H][Wd], Wd = ceil(W / 32); pixel x is bit x % 32 (LSB first) of word x / 32; the padding
 * bits of a row's last word are always WRITTEN as 0 and never trusted on input (they are masked where they could matter).
 * Images are uint8 [B][H][W][3] (what a PNG holds and sidlsg_control_hint_u8 takes), B H W 3 < 2^31.
 * sidlsg_canny_classify_u8: images + thresholds 0 <= low <= high -> planes cand and strong.  One launch: a 64 x 16 tile with a halo of
 *   2 in LDS, one lane per pixel, the planes written from wave64 ballots (no byte map exists in memory).  Per pixel:
 *     Sobel      per channel, 3 x 3: dx = (p[y-1][x+1] + 2 p[y][x+1] + p[y+1][x+1]) - (the same at x-1), dy = (p[y+1][x-1] + 2 p[y+1][x]
 *                + p[y+1][x+1]) - (the same at y-1), in int32, the border REPLICATED.
 *     channel    the pixel takes (dx, dy) of the channel with the largest |dx| + |dy|; on a tie the first in R, G, B order.
 *     magnitude  m = |dx| + |dy| of that channel; m OUTSIDE the image is 0.
 *     candidate  m > low, and with TG22 = 13573 (= int(0.41421356.. * 2^15 + 0.5)), ax = |dx|, ay = |dy| << 15, t22 = ax * TG22,
 *                t67 = t22 + (ax << 16):
 *                  ay < t22 (horizontal gradient):  m > m[y][x-1] && m >= m[y][x+1]
 *                  ay > t67 (vertical):             m > m[y-1][x] && m >= m[y+1][x]
 *                  else (diagonal), s = ((dx ^ dy) < 0) ? -1 : 1:  m > m[y-1][x-s] && m > m[y+1][x+s]
 *                The > / >= asymmetry is part of the rule: it decides which pixel of a two-pixel plateau survives.
 *     strong     cand && m > high.
 *   SIDLSG_EINVAL, and no launch, for a NULL pointer, B, H or W < 1, low < 0 or low > high, 2^31 image bytes or more.
 * sidlsg_edge_hysteresis: edges = the unique least fixed point of E = (strong & cand) | (cand & dilate3x3(E)), 8-connectivity: the
 *   candidates connected to a strong candidate.  ONE WORKGROUP PER IMAGE with both planes in LDS (2 H Wd 4 bytes, at most 147456 = two
 *   planes of 768 x 768; sidlsg_edge_hysteresis_lds_bytes(H, W) is the host query, negative beyond the limit).  A round is bit-parallel:
 *   a word's horizontal dilation is two shifts with the carry bits of its neighbour words, the vertical one reads the rows above and
 *   below, the new bits fill their runs of candidates inside the word, then one workgroup-wide OR of "changed".  The round loop is
 *   uniform and capped at H W + 1 rounds (a productive round adds a pixel, so correct code cannot reach the cap); no host round trip,
 *   no atomics.  edges: the plane; rgb_u8: uint8 [B][H][W][3], 255 in all three channels on an edge, else 0 (what a ControlNet takes);
 *   either may be NULL, not both.  rounds: int [B] or NULL, the rounds run (the last, unproductive one included).  strong bits outside
 *   cand are ignored.  SIDLSG_EINVAL, and no launch, for NULL cand / strong, both outputs NULL, B, H or W < 1, planes beyond the limit.
 * sidlsg_edge_pack_u8: bit = any of the pixel's three channels >= threshold (0 .. 255): how a control image becomes an edge set.
 * sidlsg_edge_match_counts: planes a, b, tolerance 0 <= r <= 16 -> counts int64 [B][4] = |a|, |b|, |a & D_r(b)|, |b & D_r(a)|, D_r =
 *   r rounds of 3 x 3 dilation (Chebyshev distance <= r) CLIPPED to the image: nothing leaks from padding bits, across rows or across
 *   images.  Popcounts, added by integer atomics (an integer sum has no order) into counts, which the call zeroes first; counts 8-byte
 *   aligned.  SIDLSG_EINVAL, nothing launched and counts untouched, for NULL pointers, B, H or W < 1, r outside 0 .. 16. */
int sidlsg_canny_classify_u8(const void* images_u8, void* cand, void* strong, int B, int H, int W, int low, int high, void* stream);
int sidlsg_edge_hysteresis_lds_bytes(int H, int W);
int sidlsg_edge_hysteresis(const void* cand, const void* strong, void* edges, void* rgb_u8, int* rounds, int B, int H, int W, void* stream);
int sidlsg_edge_pack_u8(const void* images_u8, void* bits, int B, int H, int W, int threshold, void* stream);
int sidlsg_edge_match_counts(const void* a, const void* b, void* counts, int B, int H, int W, int r, void* stream);

/* ---- CLIP text encoder (sid_lsg_amd/text.py HipCLIPTextModel; transformers' CLIPTextModel, which the reference calls) ------------
 * sidlsg_attn_causal_fwd(_f32): O = softmax(mask(Q K^T D^-1/2)) V per head, key j visible to query i iff j <= i.  Forward only, no
 *   LSE.  Q/K/V/O: [B][N][ld*] views of bf16 (_f32: fp32) holding H heads of width D side by side (token stride ld* >= H * D, batch
 *   stride bs*, in elements), so a fused [B][N][3 H D] projection is consumed in place.  1 <= N <= 128 (queries = keys), D a multiple
 *   of 8 up to 128; one workgroup per (batch, head) stages K and V in LDS once, wave w owns queries 16 w .. 16 w + 15 and visits key tiles
 *   0 .. w only; single-pass softmax in fp32 (bf16: P rounded to bf16 once for the PV product; _f32: nothing rounded to bf16).
 *   SIDLSG_EINVAL, and no launch, for any other N or D, null pointers, pointers not 16-byte aligned, ld* / bs* that are not
 *   multiples of 16 bytes or ld* < H * D.
 * sidlsg_text_embed(_f32): out[b L + l][:] = tok[ids[b][l]][:] + pos[l][:].  ids int64 [B][L]; tok fp32 [V][D], pos fp32 [P][D], L <= P;
 *   out bf16 (_f32: fp32) [B L][D], the fp32 sum rounded once.  D % 8 == 0, tables and out 16-byte aligned; SIDLSG_EINVAL otherwise.  An
 *   id outside [0, V) reads nothing: its row is written as NaN. */
int sidlsg_attn_causal_fwd(const void* Q, const void* K, const void* V, void* O, int B, int H, int N, int D, int ldq, int ldk, int ldv,
                           int ldo, long long bsq, long long bsk, long long bsv, long long bso, void* stream);
int sidlsg_attn_causal_fwd_f32(const void* Q, const void* K, const void* V, void* O, int B, int H, int N, int D, int ldq, int ldk, int ldv,
                               int ldo, long long bsq, long long bsk, long long bsv, long long bso, void* stream);
int sidlsg_text_embed(const void* ids, const float* tok, const float* pos, void* out, int B, int L, int D, int V, int P, void* stream);
int sidlsg_text_embed_f32(const void* ids, const float* tok, const float* pos, void* out, int B, int L, int D, int V, int P, void* stream);

/* ---- HPSv2 preprocessing (sid_lsg_amd/hps.py; open_clip's validation transform, which the hpsv2 package scores through) --------
 * sidlsg_pil_patches_u8(_f32): Pillow's 8-bit BICUBIC resize of the shorter side to R, the R x R centre crop, ToTensor, Normalize and
 *   the patch unfold in one launch.  images: uint8 [B][3][H][W].  The resampling is Pillow's ImagingResample in integers: per pass
 *   clip8((2^21 + sum_k coeff[k] * in[first + k]) >> 22), horizontal pass first, the vertical pass on its 8-bit result; the
 *   intermediate picture lives in LDS only.  The 22-bit coefficient banks are built on the host in double as Pillow builds them
 *   (sid_lsg_amd.metrics.pil_crop_plan) and restricted to the crop: hbounds int32 [R][2] = (first source column, taps <= hk) of
 *   cropped output column x, hcoef int32 [R][hk]; vbounds / vcoef / vk likewise for rows; band_rows: the largest number of source
 *   rows the vertical windows of P consecutive output rows span.  A side that takes no pass has one tap of 1 << 22.  Then in fp32,
 *   exactly: (p / 255 - mean_c) / std_c, an IEEE division, a subtraction and an IEEE division; bf16 rounds that once.  out: bf16 (_f32:
 *   fp32) [B * (1 + (R/P)^2)][Kp], the layout sidlsg_clip_patches_u8 writes (column (c * P + py) * P + px; pad columns and the
 *   class-token row zero).  One workgroup per (image, row of patches); its LDS tile is 3 * band_rows * roundup(R, 4) bytes of
 *   intermediate picture behind a 3 KiB table and must fit 64 KiB: 3072 + 3 * band_rows * roundup(R, 4) <= 65536 (224 / 14 from
 *   512^2: 38 rows, 28 KiB; from 1024^2: 78 rows, 54 KiB).  SIDLSG_EINVAL, and no launch, for a band beyond that limit, R % P != 0,
 *   Kp % 8 != 0, Kp < 3*P*P, std == 0, null pointers, out not 16-byte or a table not 4-byte aligned, hk / vk / band_rows <= 0, 2^31 or
 *   more input bytes or output elements.  Table entries are clamped to the image before use: a wrong bank cannot read outside it. */
int sidlsg_pil_patches_u8(const void* images, void* out, int B, int H, int W, int R, int P, int Kp, const int* hbounds, const int* hcoef,
                          int hk, const int* vbounds, const int* vcoef, int vk, int band_rows, float mean0, float mean1, float mean2,
                          float std0, float std1, float std2, void* stream);
int sidlsg_pil_patches_u8_f32(const void* images, void* out, int B, int H, int W, int R, int P, int Kp, const int* hbounds, const int* hcoef,
                              int hk, const int* vbounds, const int* vcoef, int vk, int band_rows, float mean0, float mean1, float mean2,
                              float std0, float std1, float std2, void* stream);

/* ---- reference plugin op: torch_utils/ops/bias_act.cpp:32 `bias_act(x,b,xref,yref,dy,grad,dim,act,alpha,gain,clamp)`
 * act: 1 linear 2 relu 3 lrelu 4 tanh 5 sigmoid 6 elu 7 selu 8 softplus 9 swish (bias_act.py:23-33).
 * grad 0: out = clamp(act(x + b[(i/stepB)%sizeB]) * gain); grad 1: out = dL/dx from dy (x, b = saved inputs).
 * dtype 0 fp32, 1 bf16. */
int sidlsg_bias_act(const void* x, const void* b, const void* dy, void* out, long long n, int stepB, int sizeB, int act,
                    float alpha, float gain, float clamp, int grad, int dtype, void* stream);

/* ---- fp8-weight contractions (BASELINE.json configs[4] "fp8 MFMA weights"; no counterpart in the reference, which only
 * knows fp32 / fp16: training/sid_training_loop.py:205) ----------------------------------------------------------------
 * For FROZEN networks: W8 = OCP e4m3 bytes [N][K] with one fp32 scale per output channel (sidlsg_quantize_fp8_rows from
 * the bf16 compute copy); A / X stay bf16 in HBM and are converted to e4m3 in the kernel's loader (static unit scale,
 * saturating); v_mfma_f32_16x16x32_fp8_fp8, fp32 accumulation, C = act(alpha * wscale[n] * acc + bias + rowvec + res).
 * Same remaining arguments as sidlsg_gemm_bf16 / sidlsg_conv3x3_bf16; K (Cin) multiple of 16.
 * NaN: every bf16 / fp32 -> e4m3 conversion of this library (sidlsg_cast_fp8, the fp8w loader, the e4m3-output norms,
 * sidlsg_quantize_fp8_rows) turns a NaN into an e4m3 NaN byte (0x7F / 0xFF), never into a clamped number: a NaN activation
 * makes every output of its row NaN.  sidlsg_quantize_fp8_rows: scale[r] = max|x| / 448 over the row's non-NaN entries (1 if
 * that maximum is 0), a NaN entry becomes a NaN byte and leaves the other bytes and the scale of its row unchanged; a row of NaN
 * only has scale 1.  An infinite entry makes the row's scale infinite, its own byte NaN and every finite entry's byte a zero of its sign. */
int sidlsg_quantize_fp8_rows(const void* src_bf16, void* dst_fp8, float* scale, int rows, int cols, void* stream);
int sidlsg_gemm_fp8w(const void* A, int lda, const void* W8, const float* wscale, void* C, int ldc, const float* bias, const void* res,
                     int ldres, const float* rowvec, int ld_rowvec, int rows_per_batch, int M, int N, int K, float alpha,
                     int flags, void* stream);
int sidlsg_conv3x3_fp8w(const void* X, int ldx, const void* W8, const float* wscale, void* Y, int ldc, const float* bias,
                        const void* res, int ldres, const float* rowvec, int ld_rowvec, int B, int H, int Wd, int Cin, int Cout,
                        int stride, int ups, float alpha, int flags, void* stream);
/* Both operands e4m3 (MX MFMA v_mfma_scale_f32_16x16x128_f8f6f4 with unit block scales: twice the bf16 rate on gfx950).
 * A8: e4m3 bytes [M][lda] at unit scale -- what the GroupNorm / LayerNorm kernels write with an e4m3 output
 * (sidlsg_cast_fp8 converts a bf16 matrix: clamp to +-448, round to nearest even); W8 / wscale as above.  N % 160 == 0,
 * K % 16 == 0, lda % 16 == 0; the epilogue arguments are those of sidlsg_gemm_bf16.  sidlsg_cast_fp8: n % 8 == 0; a NaN
 * element becomes an e4m3 NaN byte ("NaN" under "fp8-weight contractions" above). */
int sidlsg_cast_fp8(const void* src_bf16, void* dst_fp8, long long n, void* stream);
/* conv3x3, pad 1, stride 1 on an e4m3 NHWC image (X8: [B][H][Wd][ldx] bytes); W8: [Cout][9 * Cin] e4m3; Cin % 16 == 0,
 * Cout % 160 == 0; rowvec: the per-image row vector (time-embedding broadcast), one row per image. */
int sidlsg_conv3x3_mx8(const void* X8, int ldx, const void* W8, const float* wscale, void* Y, int ldc, const float* bias, const void* res,
                       int ldres, const float* rowvec, int ld_rowvec, int B, int H, int Wd, int Cin, int Cout, float alpha, int flags,
                       void* stream);
/* sidlsg_layernorm_fwd / sidlsg_groupnorm_fwd on bf16 x with y8 written as e4m3 bytes at unit scale (clamped to +-448, round to
 * nearest even); stats as in the bf16 forms.  A NaN in x makes every y8 byte of its row / (sample, group) an e4m3 NaN byte ("NaN"
 * under "fp8-weight contractions" above). */
int sidlsg_layernorm_fwd_fp8(const void* x, const float* gamma, const float* beta, void* y8, float* stats, int rows, int C,
                             float eps, void* stream);
int sidlsg_groupnorm_fwd_fp8(const void* x, const float* gamma, const float* beta, void* y8, float* stats, float* ws, int B,
                             int HW, int C, int G, float eps, int silu, void* stream);
int sidlsg_gemm_mx8(const void* A8, int lda, const void* W8, const float* wscale, void* C, int ldc, const float* bias, const void* res,
                    int ldres, const float* rowvec, int ld_rowvec, int rows_per_batch, int M, int N, int K, float alpha,
                    int flags, void* stream);
/* Grouped forms of the e4m3 entry points ("grouped launches" above: two FROZEN networks that both hold e4m3 copies of the same
 * layers, one stacked batch).  Rows (samples) of the first half use (W8, wscale, bias) resp. (gamma, beta), those of the second
 * half (W8_1, wscale1, bias1) resp. (gamma1, beta1); res / rowvec / outputs are stacked like the input.  M (B, rows) even, bias
 * and bias1 both given or both NULL, every set starts on a tile boundary of its own (the halves need not be tile aligned).
 * Otherwise the arguments and restrictions of the ungrouped entry points; the layer's backward-data pass is the bf16 grouped
 * entry point on the transposed bf16 copies. */
int sidlsg_gemm_fp8w_g2(const void* A, int lda, const void* W8, const float* wscale, const void* W8_1, const float* wscale1, void* C, int ldc,
                        const float* bias, const float* bias1, const void* res, int ldres, const float* rowvec, int ld_rowvec,
                        int rows_per_batch, int M, int N, int K, float alpha, int flags, void* stream);
int sidlsg_conv3x3_fp8w_g2(const void* X, int ldx, const void* W8, const float* wscale, const void* W8_1, const float* wscale1, void* Y, int ldc,
                           const float* bias, const float* bias1, const void* res, int ldres, const float* rowvec, int ld_rowvec, int B, int H,
                           int Wd, int Cin, int Cout, int stride, int ups, float alpha, int flags, void* stream);
int sidlsg_gemm_mx8_g2(const void* A8, int lda, const void* W8, const float* wscale, const void* W8_1, const float* wscale1, void* C, int ldc,
                       const float* bias, const float* bias1, const void* res, int ldres, const float* rowvec, int ld_rowvec,
                       int rows_per_batch, int M, int N, int K, float alpha, int flags, void* stream);
int sidlsg_conv3x3_mx8_g2(const void* X8, int ldx, const void* W8, const float* wscale, const void* W8_1, const float* wscale1, void* Y, int ldc,
                          const float* bias, const float* bias1, const void* res, int ldres, const float* rowvec, int ld_rowvec, int B, int H,
                          int Wd, int Cin, int Cout, float alpha, int flags, void* stream);
int sidlsg_groupnorm_fwd_fp8_g2(const void* x, const float* gamma, const float* beta, const float* gamma1, const float* beta1, void* y8,
                                float* stats, float* ws, int B, int HW, int C, int G, float eps, int silu, void* stream);
int sidlsg_layernorm_fwd_fp8_g2(const void* x, const float* gamma, const float* beta, const float* gamma1, const float* beta1, void* y8,
                                float* stats, int rows, int C, float eps, void* stream);

/* ---- fp32-accurate compute mode ------------------------------------------------------------------------------
 * The reference's default precision is fp32 (training/sid_training_loop.py:205 `dtype = float16 if use_fp16 else float32`,
 * run_sid.sh:63-88) and BASELINE.json configs[0] is fp32.  Every entry point above that touches bf16 activations also
 * exists with the suffix _f32: same arguments and semantics, but activations (A/X/C/Y/res, x/y/dy/dx, Q/K/V/O, ...) and
 * the compute copies of the weights (W, transposed W) are fp32 and the contractions run on the f32-input matrix
 * cores (v_mfma_f32_16x16x4_f32: exact fp32 products, fp32 accumulation).  Selected per network by
 * HipUNet2DCondition(compute_dtype=torch.float32); used by the parity suite to assert north_star's 1e-3 bound.
 * Differences: K, lda, ldx, ldy multiples of 4; flags: only SIDLSG_SILU / SIDLSG_ACCUM (C is always fp32); the
 * weight-gradient entry points take dBias = NULL (the bias gradient is a sidlsg_colsum_f32 call); no workspace is used;
 * sidlsg_transpose_w(_batched)_f32 write fp32 destinations; sidlsg_attn_fwd_f32 / _bwd_f32 take D a multiple of 4 with the
 * same round-up rule as the bf16 attention (16, 32, 48, 64, 80, 96, 128 or 160), SIDLSG_EINVAL otherwise. */
int sidlsg_gemm_f32(const void* A, int lda, const void* W, void* C, int ldc, const float* bias, const void* res, int ldres,
                    const float* rowvec, int ld_rowvec, int rows_per_batch, int M, int N, int K, float alpha, int flags,
                    void* stream);
int sidlsg_conv3x3_f32(const void* X, int ldx, const void* W, void* Y, int ldc, const float* bias, const void* res, int ldres,
                       const float* rowvec, int ld_rowvec, int B, int H, int Wd, int Cin, int Cout, int stride, int ups,
                       float alpha, int flags, void* stream);
int sidlsg_wgrad_f32(const void* dY, int ldy, const void* A, int lda, float* dW, float* dBias, int M, int N, int K,
                     void* stream);
int sidlsg_conv3x3_wgrad_f32(const void* dY, int ldy, const void* X, int ldx, float* dW, float* dBias, int B, int H, int Wd,
                             int Cin, int Cout, int stride, int ups, void* stream);
int sidlsg_groupnorm_fwd_f32(const void* x, const float* gamma, const float* beta, void* y, float* stats, float* ws, int B,
                             int HW, int C, int G, float eps, int silu, void* stream);
int sidlsg_groupnorm_bwd_f32(const void* x, const void* dy, const float* stats, const float* gamma, const float* beta,
                             const void* dres, void* dx, float* dgamma, float* dbeta, float* ws, int B, int HW, int C, int G,
                             int silu, void* stream);
int sidlsg_layernorm_fwd_f32(const void* x, const float* gamma, const float* beta, void* y, float* stats, int rows, int C,
                             float eps, void* stream);
int sidlsg_layernorm_bwd_f32(const void* x, const void* dy, const float* stats, const float* gamma, const void* dres, void* dx,
                             float* dgamma, float* dbeta, float* ws, int rows, int C, void* stream);
int sidlsg_attn_fwd_f32(const void* Q, const void* K, const void* V, void* O, float* LSE, int B, int H, int Nq, int Nk, int D,
                        int ldq, int ldk, int ldv, int ldo, long long bsq, long long bsk, long long bsv, long long bso,
                        void* stream);
int sidlsg_attn_bwd_f32(const void* Q, const void* K, const void* V, const void* O, const void* dO, const float* LSE, void* dQ,
                        void* dK, void* dV, float* delta, int B, int H, int Nq, int Nk, int D, int ldq, int ldk, int ldv,
                        int ldo, long long bsq, long long bsk, long long bsv, long long bso, void* stream);
int sidlsg_noisy_input_f32(const float* x0, const float* noise, const float* s0, const float* s1, void* out, float* xt, int B,
                           int C, int HW, int Cp, int dup, void* stream);
int sidlsg_noisy_input_bwd_f32(const void* g, const float* s0, float* dx0, int B, int C, int HW, int Cp, int dup,
                               int accumulate, void* stream);
int sidlsg_cfg_x0_bwd_f32(const float* g, const float* s0, const float* s1, void* deps, float* dxt, int B, int C, int HW,
                          int Cp, int dup, float kappa, int mode, void* stream);
int sidlsg_step_renoise_f32(const float* eps, const float* xt, const float* s0, const float* s1, const float* s0n,
                            const float* s1n, const float* noise, void* out, float* xtn, int B, int C, int HW, int Cp, int mode,
                            void* stream);
int sidlsg_step_renoise_bwd_f32(const void* g, const float* gxtn, const float* s0, const float* s1, const float* s0n, void* deps,
                                float* dxt, int B, int C, int HW, int Cp, int mode, void* stream);
int sidlsg_ddim_step_f32(const float* eps, const float* xt, const float* s0, const float* s1, const float* s0p, const float* s1p,
                         void* out, float* xtn, float* x0, int B, int C, int HW, int Ce, int Cp, int dup, float kappa, int mode,
                         void* stream);
int sidlsg_solver_step_f32(const float* eps, const float* xt, const float* s0, const float* s1, const float* coef, const float* x0p,
                           const float* noise, const float* scale, void* out, float* xtn, float* x0, int B, int C, int HW, int Ce,
                           int Cp, int dup, float kappa, int mode, int need_prev, void* stream);
int sidlsg_masked_renoise_f32(const float* x, const float* z0, const float* noise, const unsigned char* mask, const float* a0,
                              const float* a1, void* out, float* xn, int B, int C, int HW, int Cp, int dup, int mask_shared,
                              void* stream);
int sidlsg_timestep_embed_f32(const long long* t, void* out, int B, int dim, void* stream);
int sidlsg_silu_fwd_f32(const void* x, void* y, long long n, void* stream);
int sidlsg_silu_bwd_f32(const void* x, const void* dy, void* dx, long long n, void* stream);
int sidlsg_geglu_fwd_f32(const void* h, void* y, long long M, int F, void* stream);
int sidlsg_geglu_bwd_f32(const void* h, const void* dy, void* dh, long long M, int F, void* stream);
int sidlsg_concat2_f32(void* a, void* b, void* out, long long M, int C1, int C2, int to_parts, void* stream);
int sidlsg_sumpool2x2_f32(const void* g, void* out, int B, int H, int W, int C, void* stream);
int sidlsg_zero_insert2_f32(const void* g, void* out, int B, int Ho, int Wo, int H, int W, int C, void* stream);
int sidlsg_add_f32(const void* a, const void* b, void* o, long long n, void* stream);
int sidlsg_colsum_f32(const void* g, int ldg, float* per_batch, float* total, float* ws, int B, int rows_per_batch, int N,
                      void* stream);
int sidlsg_colsum_strided_f32(const void* g, int ldg, float* per_batch, int ld_pb, float* total, int B, int rows_per_batch, int N, void* stream);
int sidlsg_transpose_w_f32(const float* src, void* dst, int N, int K, int T, void* stream);
int sidlsg_transpose_w_batched_f32(const void* jobs, int njobs, int nblocks, void* stream);

#ifdef __cplusplus
}
#endif
#endif
