/* hfa.h — C ABI of libhfa.so: hand-written gfx950 (MI355X, CDNA4) kernels for the HubertFA inference path.
 *
 * Conventions (all entry points):
 *   - return 0 on success, HFA_EINVAL (-1000) on a bad argument, -(hipError_t) on a HIP launch error;
 *     hfa_last_error() gives the calling thread's last message.
 *   - every pointer is a DEVICE pointer owned by the caller (except the host-side WAV reader's), the library
 *     never allocates persistent memory and never frees caller memory.
 *   - stream-ordered on `stream`, no implicit synchronisation, re-entrant across streams/threads, so every
 *     call can be captured into a hipGraph.  The *_tuning hooks (benchmark overrides) set state of the calling
 *     thread only (thread-local), so they never change another thread's launches.
 *   - plain pointers and sizes only (no torch types); layouts are row-major with the strides named.
 *
 *   - variable-length batches: the optional `const int32_t*` length arrays ([B], device) give each row's own
 *     length; statistics (GroupNorm, conv0's GroupNorm, wave normalisation) and attention keys cover that
 *     length only, and padding rows come out as zeros (or don't-care where stated), so every utterance gets
 *     the result it would get alone — the reference runs one utterance at a time.  NULL = all rows full.
 *
 * Each entry cites the reference interface it replaces (paths relative to the HubertFA repository).
 */
#ifndef HFA_H_
#define HFA_H_

#include <stdint.h>
#include <hip/hip_runtime_api.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HFA_EINVAL (-1000)

/* ---- library ------------------------------------------------------------------------------------------- */
const char* hfa_last_error(void);
/* HFA_ABI_VERSION: bumped on every incompatible change of an entry point's arguments or of the set of entry points
 * (INTEGRATION.md §4 lists the changes); bindings check hfa_abi_version() == the version they were written for. */
#define HFA_ABI_VERSION 2
int hfa_abi_version(void);
const char* hfa_build_arch(void);

/* ---- WAV front end (hubertfa_amd/csrc/wav.cpp; HOST memory, no stream, never touches the GPU) ----------------
 * Replace torchaudio.load in tools/load_wav.py:5 (default normalize=True): RIFF/WAVE, PCM 8/16/24/32-bit or IEEE
 * float 32/64, plain or WAVE_FORMAT_EXTENSIBLE; samples scaled as torchaudio (uint8 (x-128)/128, int16 / 2^15,
 * 24-bit / 2^23, int32 / 2^31, f64 rounded to f32).  A data chunk longer than the file ends at end of file.
 * hfa_wav_info reads the headers only (frames per channel, channels, sample rate): the length-sorted batch plan
 * and the multi-GPU shard costs need every file's length before any is decoded.
 * hfa_wav_read decodes channel `channel` (0-based; the reference keeps waveform[0]) into dst[frames], or every
 * channel planar into dst[channels][frames] with channel = -1; `capacity` is dst's size in floats (HFA_EINVAL
 * if the samples do not fit).  `path` is a NUL-terminated file name; both are re-entrant. */
int hfa_wav_info(const char* path, int64_t* frames, int32_t* channels, int32_t* sample_rate);
int hfa_wav_read(const char* path, int32_t channel, float* dst, int64_t capacity, int64_t* frames,
                 int32_t* sample_rate);

/* ---- alignment decoder (hubertfa_amd/csrc/viterbi.hip) ------------------------------------------------------
 * hfa_viterbi_forward replaces AlignmentDecoder.forward_pass, tools/alignment_decoder.py:170-230 (numba JIT),
 * batched: utterance b has T[b] frames and S[b] states inside [Tmax, Smax] planes.
 *   prob_log [B,Tmax,Smax] f32, not_edge_log/edge_log [B,Tmax] f32, ph_seq_id [B,Smax] i32,
 *   curr [B,Smax] f64 (in/out, = curr_ph_max_prob_log), dp [B,Tmax,Smax] f32 (row 0 in, rows 1.. out),
 *   bt [B,Tmax,Smax] i8 (rows 1.. out; = backtrack_s), prob3_pad_len [B] i32 or NULL (=2 if S>=2 else 1).
 * Bit-exact with the reference (f32 sums, f64 curr*(T/S) term, strict '>' ties stay->advance->skip).
 * Smax <= 32768 (one wave up to 512 states, then 2-8 states per lane over up to 16 waves to 8192 states, then the
 * state range as segments of 8192 walked in order inside each time step). */
int hfa_viterbi_forward(int B, int Tmax, int Smax, const int32_t* T, const int32_t* S,
                        const int32_t* prob3_pad_len, const float* prob_log, const float* not_edge_log,
                        const float* edge_log, double* curr, float* dp, int8_t* bt, const int32_t* ph_seq_id,
                        hipStream_t stream);

/* The same DP over time steps [t_begin, t_end) only (t_begin >= 1; clipped to each utterance's T[b]): it continues
 * from dp row t_begin - 1 and from curr, and leaves curr for the next range, so consecutive ranges give the bits of
 * one whole call.  Lets the caller cut a long lattice (config 5: 25 839 steps, 13 ms on one CU) into pieces that
 * run beside the next batch's attention kernels.  Smax > 8192 (the segmented-state form): whole ranges only. */
int hfa_viterbi_forward_steps(int B, int Tmax, int Smax, const int32_t* T, const int32_t* S,
                              const int32_t* prob3_pad_len, const float* prob_log, const float* not_edge_log,
                              const float* edge_log, double* curr, float* dp, int8_t* bt, const int32_t* ph_seq_id,
                              int t_begin, int t_end, hipStream_t stream);
/* The largest Smax for which hfa_viterbi_forward_steps takes partial step ranges (8192: past it the segmented-state
 * form runs whole lattices only); callers that cut a DP into ranges ask the library instead of repeating it. */
int hfa_viterbi_range_max_states(void);

/* Tuning hook (tests, benchmarks): states per lane of the multi-wave forward DP, 2 / 4 / 8, 0 = automatic (4 up
 * to 4096 states, then 8); the same bits whatever the choice. */
int hfa_viterbi_tuning(int force_k);

/* hfa_viterbi_backtrack replaces the backward half of AlignmentDecoder._decode,
 * tools/alignment_decoder.py:263-288: end state, serial backtrack, frame_confidence = exp(diff([0]+dp_path)).
 * Outputs: ph_idx_seq/ph_time_int [B,Tmax] i32 (first n_out[b] valid, ascending t), frame_conf [B,Tmax] f32.
 * Smax <= 32768; any Tmax (past 64000 frames the chased path is kept in frame_conf's buffer instead of LDS). */
int hfa_viterbi_backtrack(int B, int Tmax, int Smax, const int32_t* T, const int32_t* S, const float* dp,
                          const int8_t* bt, const int32_t* ph_seq_id, int32_t* ph_idx_seq, int32_t* ph_time_int,
                          int32_t* n_out, float* frame_conf, hipStream_t stream);

/* hfa_lattice_prologue replaces the device half of AlignmentDecoder.decode, tools/alignment_decoder.py:35-84,
 * and _decode's lattice prep :239-242.  frame_logits row (b,t) at frame_logits + b*frame_bs + t*frame_ld
 * (V contiguous floats); edge logit at edge_logits + b*edge_bs + t*edge_ld.
 * Outputs: prob_log [B,Tmax,Smax] (= ph_prob_log[:, ph_seq_id]), edge_log/not_edge_log [B,Tmax] f32,
 * edge_diff [B,Tmax] f32, edge_prob [B,Tmax] f64 (may be NULL), ph_prob_log/ph_frame_pred [B,Tmax,V] (may be
 * NULL).  V <= 1024.  dp [B,Tmax,Smax] f32 / curr [B,Smax] f64 (both or neither): also _decode's DP
 * initialisation, tools/alignment_decoder.py:244-254 (dp row 0 and curr, as hfa_viterbi_init), from frame 0's
 * lattice row, so hfa_viterbi_forward can follow directly. */
int hfa_lattice_prologue(int B, int Tmax, int V, int Smax, const int32_t* T, const int32_t* S,
                         const float* frame_logits, long long frame_ld, long long frame_bs,
                         const float* edge_logits, long long edge_ld, long long edge_bs, const int32_t* ph_seq_id,
                         float* ph_prob_log, float* ph_frame_pred, float* prob_log, float* edge_log,
                         float* not_edge_log, float* edge_diff, double* edge_prob, float* dp, double* curr,
                         hipStream_t stream);
/* hfa_viterbi_init replaces _decode's initialisation, tools/alignment_decoder.py:244-254, for a lattice that did not
 * come through hfa_lattice_prologue: dp[b,0,0] = curr[b,0] = prob_log[b,0,0]; if ph_seq_id[b,0] == 0 and S[b] > 1
 * also dp[b,0,1] = curr[b,1] = prob_log[b,0,1]; every other dp[b,0,s] and curr[b,s] (s < Smax) = -inf; T[b] = 0:
 * the whole row -inf. */
int hfa_viterbi_init(int B, int Tmax, int Smax, const int32_t* T, const int32_t* S, const float* prob_log,
                     const int32_t* ph_seq_id, float* dp, double* curr, hipStream_t stream);

/* ---- dense contractions (hubertfa_amd/csrc/gemm.hip): f32 MFMA implicit GEMM ---------------------------------
 * C[z](m,n) = epi(sum_k A[z](m,k) W[z](n,k) + bias[zg*sBg + n]) + R[z](m,n),  z = zb*G + zg,
 * A[z](m,k): k = j*Cg + c, t = m*stride + j - pad, value X[zb*sAb + zg*sAg + t*ldx + c] if 0 <= t < Tin else 0.
 * W[z] row n at W + zg*sWg + n*ldw (K contiguous, conv weights in [Cout][k][Cin] im2col order).
 * epilogue: 0 none, 1 erf-GELU (applied before the residual add).  K % 16 == 0, Cg % 16 == 0, Cg | K.
 * Replaces ATen addmm (nn.Linear) and conv1d on the path:
 *   networks/hubert/model.py:100-114 (conv1-6), :122 (projection), :135-147 (grouped positional conv),
 *   :27-33 (nn.TransformerEncoderLayer in/out proj, linear1/2), transformers HubertAttention/HubertFeedForward,
 *   networks/layer/block/resnet_block.py:17-40 (k3 convs :18-24,27-33, shortcut :36-40), networks/layer/scaling/stride_conv.py:23-47
 *   (k2 s2 conv, ConvTranspose), networks/task/forced_alignment.py:53-55 (head). */
int hfa_conv_gemm_f32(int M, int N, int K, int Zb, int G, const float* A, long long sAb, long long sAg, int ldx,
                      int stride, int pad, int Cg, int Tin, const float* W, long long sWg, int ldw,
                      const float* bias, long long sBg, const float* R, long long sRb, long long sRg, int ldr,
                      float* C, long long sCb, long long sCg, int ldc, int epilogue, hipStream_t stream);
/* Tuning hook for benchmarks: force the staging pipeline of hfa_conv_gemm_f32 (16/32 = register-staged K-step,
 * 102/103 = LDS-DMA with 2/3 stages) and the tile configuration (1..7, see gemm.hip); 0 = automatic. */
int hfa_gemm_tuning(int force_pipe, int force_cfg);
/* Name (rocprof symbol stem) of the kernel instantiation hfa_conv_gemm_f32 launches for the same arguments, e.g.
 * "gemm_dma_kernel<1, 128, 128, 2, 2, 2, 4, true>"; thread-local storage, valid until the next call. */
const char* hfa_gemm_kernel_name(int M, int N, int K, int Zb, int G, const float* A, long long sAb, long long sAg,
                                 int ldx, int stride, int pad, int Cg, int Tin, const float* W, long long sWg, int ldw,
                                 const float* bias, long long sBg, const float* R, long long sRb, long long sRg,
                                 int ldr, float* C, long long sCb, long long sCg, int ldc, int epilogue);
/* Plain Linear: C[M,N] = epi(A[M,K] W[N,K]^T + bias) + R. */
int hfa_gemm_f32(int M, int N, int K, const float* A, int lda, const float* W, int ldw, const float* bias,
                 const float* R, int ldr, float* C, int ldc, int epilogue, hipStream_t stream);

/* ---- split-f16 GEMM (gemm.hip gemm_split_kernel) -------------------------------------------------------------
 * The same contractions as hfa_conv_gemm_f32 with f32-class accuracy on the f16 MFMA: every f32 operand x is
 * carried as two f16 planes, x1 = f16(x) and x2 = f16((x - x1) * 2^11) (plane 1 at +sAp / +sWp / +sCp halves;
 * every stride in halves), and A.W = A1.W1 + 2^-11 (A1.W2 + A2.W1), each partial product exact in f32.
 * Requirements: K a multiple of 32, Cg a multiple of 32 (or of 8 and >= 32: per-lane tap tracking, f32 C only); A/W 16-B aligned with 8-half strides; |x| < 65504 for every split value
 * (producers raise *oflow otherwise; the caller recomputes on the f32 path) and |w| < 32 for W (the large
 * single-accumulator tiles form 2^11 * w1 in f16; an overflow there yields a non-finite result, which also raises
 * *oflow).  Output: f32 C (+R, 16-B rows), or with Cs non-NULL and C NULL split planes of epi(acc + bias) (no R),
 * or with both non-NULL the f32 C and the split planes of that same final value (dual output).  Rs (instead of
 * R, f32 C alone): the residual as split planes (plane 1 at +sRp; strides sRb, sRg, ldr in halves), added as
 * hi + 2^-11 lo -- the residual stream carried by the planes a LayerNorm already wrote for the next GEMM.
 * epilogue | HFA_GEMM_F16: opt-in fast mode -- the high planes alone, one f16 product per MAC (A1.W1, f32
 * accumulation: f16-class accuracy, about 2.5x the split rate); ignored by the grouped positional conv kernels
 * (Cg not a multiple of 32 or N = 48/64 windows), which keep the three products. */
#define HFA_GEMM_F16 0x100
int hfa_conv_gemm_split(int M, int N, int K, int Zb, int G, const uint16_t* A, long long sAp, long long sAb,
                        long long sAg, int ldx, int stride, int pad, int Cg, int Tin, const uint16_t* W,
                        long long sWp, long long sWg, int ldw, const float* bias, long long sBg, const float* R,
                        long long sRb, long long sRg, int ldr, const uint16_t* Rs, long long sRp, float* C,
                        uint16_t* Cs, long long sCp, long long sCb, long long sCg, int ldc, int epilogue, int* oflow,
                        hipStream_t stream);
/* rocprof symbol stem of the split instantiation for an M x N x K contraction over Z = Zb*G (out_split: planes out;
 * stride 1 assumed, as the grouped positional conv's window kernel needs). */
const char* hfa_gemm_split_kernel_name(int M, int N, int K, int Z, int out_split, int epilogue, int Cg);
/* Tile override for the split GEMM (tests, benchmarks): 0 auto; 15 the N = 48 kernel (16x16x32 MFMA; chosen
 * automatically for N = 48 with f32 output, e.g. the grouped positional conv at Cg = 48); 16 the LDS-window
 * positional conv kernel; 17 / 18 / 19 / 20 the 256x256 / 128x128 / 128x64 / 256x64 tiles; 23 / 24 256x192 /
 * 192x256 (one round of 252 tiles for N = 768 at B*T = 15968 rows); 25 128x192 with two workgroups per CU.  Every
 * tile is a single-accumulator v_mfma_f32_16x16x32_f16 tile, so results do not depend on the tile.  Other values
 * (the retired tuning-only tiles 1-14, 21, 22, 26) return HFA_EINVAL and leave the override unchanged. */
int hfa_gemm_split_tuning(int cfg);
/* x [rows, cols] f32 (row stride ldx) -> split planes y (row stride ldy, plane 1 at +sp); raises *oflow (if
 * non-NULL) for |x| >= 65504 or a non-finite x. */
int hfa_split_f16(int rows, int cols, const float* x, long long ldx, uint16_t* y, long long ldy, long long sp,
                  int* oflow, hipStream_t stream);

/* ---- attention (hubertfa_amd/csrc/attention.hip) -----------------------------------------------------------
 * O = softmax(scale * Q K^T) V per (batch, head), head_dim 64, fp32 MFMA flash attention.
 * Q(b,h,i,d) at q + b*q_bs + i*q_ld + h*64 + d (same for k, v, o).
 * With key_len, O rows i >= key_len[b] (padding queries) are written as zeros.
 * Replaces nn.MultiheadAttention/SDPA in networks/hubert/model.py:27-32 and transformers
 * modeling_hubert.py HubertAttention (eager_attention_forward). */
int hfa_attention_f32(int B, int H, int L, int head_dim, float scale, const float* q, long long q_bs, int q_ld,
                      const float* k, long long k_bs, int k_ld, const float* v, long long v_bs, int v_ld, float* o,
                      long long o_bs, int o_ld, const int32_t* key_len, hipStream_t stream);
/* The same attention on split-f16 planes (see hfa_conv_gemm_split): Q, K, V read as plane pairs (plane 1 at
 * +q_sp / +k_sp / +v_sp halves), O written as plane pairs (+o_sp); every contraction is three exact f16 MFMA
 * products (f32-class accuracy).  Pointers 16-B aligned, strides multiples of 8 halves; |O| <= max |V|. */
int hfa_attention_split(int B, int H, int L, int head_dim, float scale, const uint16_t* q, long long q_sp,
                        long long q_bs, int q_ld, const uint16_t* k, long long k_sp, long long k_bs, int k_ld,
                        const uint16_t* v, long long v_sp, long long v_bs, int v_ld, uint16_t* o, long long o_sp,
                        long long o_bs, int o_ld, const int32_t* key_len, hipStream_t stream);
/* Waves (x 32 queries) per workgroup of hfa_attention_split: 4 or 8, 0 = automatic (the form whose grid gives the
 * busiest CU fewer query rows; on a tie 8 from 2048 keys).  Results do not depend on it (every query row sees the
 * same tiles in the same order). */
int hfa_attention_split_tuning(int waves);
/* MFMA form of hfa_attention_split (tuning / A-B; 0 = automatic = 16): 16 = v_mfma_f32_16x16x32_f16, 32 =
 * v_mfma_f32_32x32x16_f16 (the round-2..5 kernel).  The same products in the same key-tile order; outputs agree to
 * f32 rounding.  HFA_EINVAL for any other value. */
int hfa_attention_split_form(int form);
/* Name of the instantiation hfa_attention_split launches for (B, H, L) under the current tuning (profiler labels). */
const char* hfa_attention_split_kernel_name(int B, int H, int L);

/* ---- normalisation (hubertfa_amd/csrc/norm.hip); act: 0 none, 1 erf-GELU, 2 Hardswish -----------------------
 * y = act(LayerNorm(x (+ res)) * gamma + beta) over rows of C <= 4096 (C % 4 == 0).
 * Replaces LayerNorm in networks/hubert/model.py:25,121 and nn.TransformerEncoderLayer norm1/2,
 * transformers HubertFeatureProjection/HubertEncoder(*StableLayerNorm)/HubertLayerNormConvLayer,
 * networks/layer/block/resnet_block.py:42-45 (LN + Hardswish). */
int hfa_layernorm_f32(int rows, int C, const float* x, long long ldx, const float* res, long long ldr,
                      const float* gamma, const float* beta, float eps, int act, float* y, long long ldy, int T,
                      const int32_t* t_len, hipStream_t stream);
/* hfa_layernorm_f32 that also writes its output as split-f16 planes (see hfa_conv_gemm_split): ys row r at
 * ys + r*ldys, plane 1 at +sps halves (8-B aligned rows), so the consuming split GEMM needs no conversion pass;
 * *oflow raised for outputs outside f16 range.  y may be NULL: planes only (the consumers read the residual from
 * them, hfa_conv_gemm_split Rs). */
int hfa_layernorm_split(int rows, int C, const float* x, long long ldx, const float* res, long long ldr,
                        const float* gamma, const float* beta, float eps, int act, float* y, long long ldy, int T,
                        const int32_t* t_len, uint16_t* ys, long long ldys, long long sps, int* oflow,
                        hipStream_t stream);
/* GroupNorm(G, C) over a channels-last [B, T, C] tensor (+act).  Replaces resnet_block.py:25-26
 * (nn.GroupNorm(16, C) + nn.Hardswish). */
int hfa_groupnorm_f32(int B, int T, int C, int G, const float* x, long long x_bs, int ldx, const float* gamma,
                      const float* beta, float eps, int act, float* y, long long y_bs, int ldy, const int32_t* t_len,
                      void* workspace, hipStream_t stream);
/* Workspace for hfa_groupnorm_f32's split-T path (long rows, few (batch, group) pairs); NULL workspace = one
 * workgroup per pair. */
long long hfa_groupnorm_workspace_bytes(int B, int T, int C, int G);
/* GroupNorm (+act) of channels-last [B, T, C] (resnet_block.py:17-26, GroupNorm(16) + Hardswish) writing f32 y
 * and / or split-f16 planes ys (plane 1 at +sps halves; the next split GEMM's operand: the UNet block's second conv);
 * C % 4 == 0, (C/G) % 4 == 0, C <= 1024, G <= 64; workspace = hfa_groupnorm_workspace_bytes(B, T, C, G) bytes; rows
 * t >= t_len[b] are zeros and excluded from the statistics; *oflow raised for a plane value out of f16 range. */
int hfa_groupnorm_split(int B, int T, int C, int G, const float* x, long long x_bs, int ldx, const float* gamma,
                        const float* beta, float eps, int act, float* y, long long y_bs, int ldy, const int32_t* t_len,
                        uint16_t* ys, long long ys_bs, int ldys, long long sps, int* oflow, void* workspace,
                        hipStream_t stream);

/* ---- extractor conv0 (hubertfa_amd/csrc/conv.hip) ------------------------------------------------------------
 * x [B, N] -> y [B, T0, 512] channels-last, T0 = (N-10)/5+1.  norm=1: GroupNorm(512,512) + GELU
 * (networks/hubert/model.py:98-99,108; transformers HubertGroupNormConvLayer), needs a workspace of
 * hfa_conv0_workspace_bytes(B, N).  norm=0: conv + bias only (HubertLayerNormConvLayer's conv). */
long long hfa_conv0_workspace_bytes(int B, int N);
int hfa_conv0_f32(int B, int N, const float* x, long long x_bs, const float* w0, const float* bias, int norm,
                  const float* gamma, const float* beta, float eps, void* workspace, float* y, long long y_bs,
                  const int32_t* t0_len, hipStream_t stream);
/* hfa_conv0_f32 with the output written as split-f16 planes (see hfa_conv_gemm_split): ys [2][B][T0][512],
 * batch stride y_bs and plane stride y_sp in halves; *oflow raised for outputs outside f16 range. */
int hfa_conv0_split(int B, int N, const float* x, long long x_bs, const float* w0, const float* bias, int norm,
                    const float* gamma, const float* beta, float eps, void* workspace, uint16_t* ys, long long y_bs,
                    long long y_sp, int* oflow, const int32_t* t0_len, hipStream_t stream);

/* ---- glue (hubertfa_amd/csrc/misc.hip) -----------------------------------------------------------------------
 * Nearest-frame gather onto the DP grid, tools/encoder.py:56-59: idx[k] = min(rint(f32(ratio)*k), U-1),
 * out[b,k,:] = units[b,idx[k],:] for k < n_frames, zero rows up to T_pad (unet.py:103-106 padding). */
int hfa_units_gather_f32(int B, int U, int C, const float* units, long long u_bs, int u_ld, int n_frames, int T_pad,
                         float ratio, float* out, long long o_bs, int o_ld, const int32_t* n_frames_b,
                         const int32_t* U_b, hipStream_t stream);
/* Wav2Vec2FeatureExtractor zero-mean/unit-variance normalisation (tools/encoder.py:94-95), f64 statistics over each
 * row's own lens[b] samples; workspace: hfa_wav_normalize_workspace_bytes(B) bytes of device memory (row partials). */
long long hfa_wav_normalize_workspace_bytes(int B);
int hfa_wav_normalize_f32(int B, int N, const float* x, long long x_bs, float eps, float* y, long long y_bs,
                          const int32_t* lens, void* workspace, hipStream_t stream);
/* Zero rows t >= lens[b] of a [B, T, C] tensor (row t of batch b at x + b*x_bs + t*ldx): the padding rows of a
 * variable-length batch, which padded convs must read as zeros (reference: each utterance runs alone, B=1). */
int hfa_mask_rows_f32(int B, int T, int C, float* x, long long x_bs, int ldx, const int32_t* lens,
                      hipStream_t stream);
/* Zero padding of rows (networks/hubert/model.py:77 F.pad 40/40; resampler edge padding). */
int hfa_pad_rows_f32(int B, int N, const float* x, long long x_bs, int left, int N_out, float* y, long long y_bs,
                     hipStream_t stream);
/* Self-test: y_nb = the branch-free erf of every GELU epilogue, y_ref = device erff (must be bit-identical). */
int hfa_selftest_erf(long long n, const float* x, float* y_nb, float* y_ref, hipStream_t stream);
/* Self-test: y = the GELU applied by every fused epilogue (GEMM, LayerNorm/GroupNorm act, conv0). */
int hfa_selftest_gelu(long long n, const float* x, float* y, hipStream_t stream);
/* Range-guard bookkeeping (no reference counterpart: the split-f16 arithmetic's per-batch overflow flags): snap[i] =
 * flags[i], then flags[i] = 0, for i < n, stream-ordered (the batch's snapshot travels with its outputs). */
int hfa_flag_take(int n, int* flags, int* snap, hipStream_t stream);
/* Workgroup cap (no reference counterpart; 0 = none, the default) for this host thread's later launches of the
 * row-streaming kernels -- hfa_split_f16, hfa_layernorm_f32 / _split, hfa_lattice_prologue, hfa_ctc_prologue,
 * hfa_ctc_grad, hfa_fa_frame_loss, hfa_fa_loss_reduce, hfa_wgrad_f32: a capped launch runs its
 * rows in a grid-stride loop over at most `wgs` workgroups (results identical).  The pipelined step enqueues its side
 * pass (UNet head + lattice, beside the next batch's encoder) under a cap: its tens of thousands of one-row
 * workgroups otherwise cost the encoder more than their work. */
int hfa_set_grid_cap(int wgs);
/* out = a + b (UNet skip connection, networks/layer/backbone/unet.py:114). */
int hfa_add_f32(long long n, const float* a, const float* b, float* out, hipStream_t stream);
/* torchaudio.transforms.Resample (sinc_interp_hann) as pad + MFMA GEMM (tools/load_wav.py:7,
 * tools/encoder.py:46-48).  orig/newr gcd-reduced; kernel [newr][Kpad]; y_bs >= (N/orig+1)*newr. */
/* The resampler on the split-f16 GEMM (f32-class): x padded and split into the workspace, then one split GEMM with
 * 16-B aligned rows.  G = 1 for orig % 8 == 0 (frame f at f * orig), G = 8 for orig % 8 == 1 (e.g. 44100 -> 16000:
 * frames 8m+g as 8 groups, group g's taps shifted right by g): Wg is [2][G][new][Kg] split planes of those taps
 * (Kg % 32 == 0, Kg >= 2 width + orig + G - 1).  y: F*new (G = 1) or ceil(F/8)*8*new (G = 8) floats per row;
 * the valid length is ceil(new*N/orig).  *oflow as hfa_split_f16. */
long long hfa_resample_split_workspace_bytes(int B, int N, int orig, int Kg, int G);
int hfa_resample_split(int B, int N, const float* x, long long x_bs, int orig, int newr, const uint16_t* Wg, int Kg,
                       int G, int width, void* workspace, float* y, long long y_bs, int* oflow, hipStream_t stream);
/* The composite of two sinc stages that return to the input rate (16 k -> 44.1 k -> 16 k: tools/load_wav.py:7 then
 * tools/encoder.py:46-48) runs as ONE hfa_resample_split pass (orig = newr = P, the composed taps); this entry
 * overwrites the output frames that pass cannot express -- those whose second-stage window reaches past the
 * intermediate row, where each stage alone zero-pads: the first ceil(wd_width / Q) frames and the frames from
 * ceil((len_u - (kwd - 1 - wd_width)) / Q) to the row's last output, computed as the two stages compute them
 * (f32): each frame's intermediate window into the workspace (hfa_resample_chain_edges_workspace_bytes), then the
 * frame's outputs.  P, Q: the first stage's gcd-reduced orig / new (the second's new / orig); wu_t [kwu][Q] and wd_t
 * [kwd][P] the stages' f32 taps, k-major; lens [B] per-row input lengths (NULL: N); len_u and the row's output
 * length follow torchaudio's float32-quotient ceil.  y: [B][y_bs] (y_cols columns exist); kwd + 512 floats fit
 * 64 KiB. */
long long hfa_resample_chain_edges_workspace_bytes(int B, int Q, int kwd, int wd_width);
int hfa_resample_chain_edges(int B, int N, const int32_t* lens, const float* x, long long x_bs, int P, int Q,
                             const float* wu_t, int kwu, int wu_width, const float* wd_t, int kwd, int wd_width,
                             void* workspace, float* y, long long y_bs, int y_cols, hipStream_t stream);
long long hfa_resample_workspace_bytes(int B, int N, int orig, int Kpad);
int hfa_resample_f32(int B, int N, const float* x, long long x_bs, int orig, int newr, const float* kernel, int Kpad,
                     int width, void* workspace, float* y, long long y_bs, hipStream_t stream);

/* ---- log-mel spectrogram (hubertfa_amd/csrc/melspec.hip) --------------------------------------------------------
 * Replaces MelSpecExtractor.__call__, tools/get_melspec.py:28-54 (torchaudio MelSpectrogram: zero padding n_fft/2,
 * STFT center=False, periodic Hann window of win_length centred in n_fft, magnitude, htk mel filterbank norm=None,
 * log(clamp(., clamp))) as ONE kernel on the split-f16 MFMA (see hfa_conv_gemm_split): x [B, N] f32 (row stride x_bs,
 * a multiple of 4; split into planes on load) -> y[b, m, f] at y + b*y_bs + m*y_ld + f for m < n_mels, f < frames.
 * Row b's own length is lens[b] (NULL: N): samples outside [0, lens[b]) read as zeros whatever the buffer holds, frames
 * f >= lens[b]/hop + 1 are written as zeros.  Tables (hubertfa_amd/melspec.py builds them from the f32 window and the
 * f32 filterbank, angles in f64), both as split planes in MFMA fragment order, element (lane, j) of a 16-row x 32-deep
 * block = [row lane & 15][k 8 (lane >> 4) + j]:
 *   basis [2][nb_pad/8 column blocks][Kpad/32][64][8]: column block 2g + part holds w[k] cos (part 0) / -w[k] sin
 *         (part 1) (2 pi (k + (n_fft - win_length)/2) bin / n_fft) of the 16 needed bins 16g .. 16g + 15 (first needed
 *         bin = the first with a non-zero filterbank row), K = win_length padded with zeros to Kpad, a multiple of 128;
 *   fb    [2][8 mel blocks][nb_pad/32][64][8]: rows mels (zeros past n_mels), k = the needed bins, nb_pad of them.
 * Envelope (else HFA_EINVAL before any launch): win_length a multiple of 32 and <= 2048, n_fft even and >= win_length,
 * hop a multiple of 8, n_mels <= 128, nb_pad a multiple of 64, x / basis / fb / y 16-B aligned.  *oflow (may be NULL)
 * is raised when a magnitude of a valid frame is not finite or >= 65504.  Results do not depend on the frame tile. */
int hfa_logmel_split(int B, int N, const float* x, long long x_bs, const int32_t* lens, int win_length, int hop,
                     int n_fft, int n_mels, int nb_pad, const uint16_t* basis, const uint16_t* fb, float clamp,
                     int frames, float* y, long long y_bs, int y_ld, int* oflow, hipStream_t stream);

/* ---- CTC head (hubertfa_amd/csrc/ctc.hip) ------------------------------------------------------------------------
 * The batched sequence likelihood and greedy decode of the head's CTC columns: F.log_softmax + nn.CTCLoss(reduction=
 * "none") of networks/task/forced_alignment.py:256-272 / networks/loss/GHMLoss.py:12-56, and AlignmentDecoder.ctc,
 * tools/alignment_decoder.py:145-150.  Utterance b has T[b] frames and L[b] target labels inside [Tmax] / [Lmax]
 * planes; frames t >= T[b] and targets j >= L[b] are never read into any result, so every utterance gets the bits it
 * gets alone.  Pointers are aligned to their element size (else HFA_EINVAL before any launch).
 *
 * hfa_ctc_prologue (one wave per frame row; honours hfa_set_grid_cap): CTC class c of frame (b,t) is read at
 * logits[b*bs + t*ld + (c == 0 ? blank_col : c + label_off)] (the head's layout: blank_col = 1, label_off = 2);
 * V <= 1024 classes.  emis [B,Tmax,Lmax+1] f32: column 0 = log_softmax(blank), column j = log_softmax(targets[b,j-1])
 * for j <= L[b] (f32 max / log-sum-exp over the V classes); best [B,Tmax] i32 = the argmax class of the raw logits,
 * the lowest class on ties (np.argmax).  targets [B,Lmax] i32 with ids in 1..V-1: the kernel trusts them, the caller
 * validates (hubertfa_amd.ops does, on the host).
 *
 * hfa_ctc_forward (one workgroup per utterance): nll[b] = -log P(targets[b,:L[b]] | frames < T[b]) as f64, from the
 * alpha recurrence over the 2L+1 extended states in f32, rebased every 16 steps against an f64 offset (DESIGN.md
 * §3.5).  An infeasible pair (T[b] < L[b] + adjacent repeats; T[b] = 0 with L[b] > 0) gives +inf, as torch with
 * zero_infinity=False; L[b] = 0 gives -sum_t emis[t,0]; T[b] = 0 and L[b] = 0 gives 0.  The state range is
 * register-resident (up to 8 label/blank pairs per lane over 16 waves): Lmax <= hfa_ctc_max_labels() = 8191, beyond
 * that HFA_EINVAL (no segmented form).
 *
 * hfa_ctc_greedy (one workgroup per utterance): ids[b,:n[b]] = best[b,t] for the frames t < T[b], ascending, with
 * best[b,t] != best[b,t-1] (best[b,-1] = 0) and best[b,t] != 0; ids [B,Tmax] i32, n [B] i32.
 *
 * Forward-backward: the state posterior gamma(t,s) = P(state s at frame t | targets, frames) =
 * exp(alpha[t,s] + beta[t,s] - y[t,s] + nll), alpha / beta in torch's convention (both include the emission y[t,s]),
 * and from it the per-label report and the gradient of the loss of forced_alignment.py:256-272 that
 * nn.CTCLoss's backward gives the reference.  The envelope is hfa_ctc_forward's.
 *
 * hfa_ctc_forward_alpha: hfa_ctc_forward (nll has the same bits) that also stores every step's alpha row, relative to
 * an f64 offset: alpha [B,Tmax,2,Lmax+1] f32, plane 0 = the blank states j <= L[b], plane 1 = the label states
 * j < L[b]; aoff [B,Tmax] f64 (8-byte aligned); true alpha = alpha + aoff[b,t], -inf = unreachable.  Rows t >= T[b]
 * and slots past L[b] are not written, except plane 1's slot L[b], which holds garbage.  B*Tmax*2*(Lmax+1)*4 bytes,
 * the caller's.
 *
 * hfa_ctc_backward (one workgroup per utterance): the mirror scan from t = T[b]-1 down, beta in f32 rebased every 16
 * steps like alpha; gamma = exp(f32(alpha_rel + beta_rel - y) + f32(aoff + boff + nll)).  Writes
 *   occ [B,Tmax,Lmax+1] f32 (emis's layout): column 0 = sum_j gamma(t, blank_j), column j = gamma(t, label_{j-1}) for
 *       j <= L[b]; zeros for t >= T[b] and j > L[b];
 *   frames [B,Lmax] = sum_t occ[t,j+1];  centre = sum_t t occ[t,j+1] / frames (in frames);
 *   logp = sum_t occ[t,j+1] emis[t,j+1] / frames (the posterior-weighted mean log-probability of label j); zeros for
 *       j >= L[b].
 * An infeasible utterance (nll = +inf) gives zeros and logp = -inf (j < L[b]); never NaN.  No atomics: every value has
 * the bits it has alone at B = 1, whatever form the batch's Lmax selects.
 *
 * hfa_ctc_grad (one wave per frame row; honours hfa_set_grid_cap): class c of frame (b,t), read as hfa_ctc_prologue
 * reads it, gets grad[b*g_bs + t*g_ld + col(c)] = w[b] (softmax(x[b,t])[c] - Gamma[t,c]) = w[b] d nll[b] / d x[b,t,c];
 * other columns are not touched; rows t >= T[b] and infeasible utterances get zeros.  Gamma of the blank is occ's
 * column 0; Gamma of class c sums occ's columns of the target positions cls_idx[b, cls_ptr[b,c] .. cls_ptr[b,c+1])
 * (cls_ptr [B,V+1], cls_idx [B,Lmax] i32: the positions j < L[b] grouped by class, ascending within a class) in that
 * order, so it is deterministic.  weight [B] f32 or NULL (= 1). */
int hfa_ctc_max_labels(void);
int hfa_ctc_prologue(int B, int Tmax, int V, int Lmax, const int32_t* T, const int32_t* L, const float* logits,
                     long long ld, long long bs, int blank_col, int label_off, const int32_t* targets, float* emis,
                     int32_t* best, hipStream_t stream);
int hfa_ctc_forward(int B, int Tmax, int Lmax, const int32_t* T, const int32_t* L, const float* emis,
                    const int32_t* targets, double* nll, hipStream_t stream);
int hfa_ctc_greedy(int B, int Tmax, const int32_t* T, const int32_t* best, int32_t* ids, int32_t* n,
                   hipStream_t stream);
int hfa_ctc_forward_alpha(int B, int Tmax, int Lmax, const int32_t* T, const int32_t* L, const float* emis,
                          const int32_t* targets, double* nll, float* alpha, double* aoff, hipStream_t stream);
int hfa_ctc_backward(int B, int Tmax, int Lmax, const int32_t* T, const int32_t* L, const float* emis,
                     const int32_t* targets, const double* nll, const float* alpha, const double* aoff, float* occ,
                     float* frames, float* centre, float* logp, hipStream_t stream);
int hfa_ctc_grad(int B, int Tmax, int V, int Lmax, const int32_t* T, const int32_t* L, const float* logits,
                 long long ld, long long bs, int blank_col, int label_off, const float* occ, const double* nll,
                 const int32_t* cls_ptr, const int32_t* cls_idx, const float* weight, float* grad, long long g_ld,
                 long long g_bs, hipStream_t stream);

/* ---- full-label alignment losses (hubertfa_amd/csrc/loss.hip) ------------------------------------------------------
 * The four full-label terms of _get_loss, networks/task/forced_alignment.py:188-254, fused, with their gradient with
 * respect to the head logits and the counts the reference's EMA tables are updated from:
 * ph_frame_GHM_loss (GHMLoss, networks/loss/GHMLoss.py:221-302), ph_edge_GHM_loss and ph_edge_diff_loss
 * (MultiLabelGHMLoss(1), GHMLoss.py:117-211, the latter on forced_alignment.py:224-236's pairs) and ph_edge_EMD_loss
 * (networks/loss/BinaryEMDLoss.py:4-15).  Conventions of the CTC block.  logits: the head's [B,Tmax,V+2] rows, frame
 * (b,t) at logits + b*bs + t*ld, column 0 the edge, column 1 never read or written, columns 2.. the V <= 1024 frame
 * classes.  Row b takes part iff label_type[b] >= 2, its frames t < T[b]; nothing else in any buffer (NaN included),
 * and no logit of a class with ph_mask[b,c] == 0, reaches any output.  ph_frame [B,Tmax] i32 (class ids; clamped to
 * 0..V-1, the caller validates), ph_edge [B,Tmax] f32 in [0,1], ph_mask [B,V] i32 (non-zero = live).
 * tables, f32 [V + 3 num_bins + 6] (num_bins <= 64), is the reference's six buffers in one array, and hist (i32) the
 * matching counts: class_ema [V] | GD_ema [num_bins] (ph_frame_GHM_loss_fn) | GD_stat_ema [num_bins] |
 * label_stat_ema_each_class [3] (ph_edge_GHM_loss_fn) | the same two of ph_edge_diff_GHM_loss_fn.
 * Loss order everywhere: 0 frame, 1 edge, 2 EMD, 3 edge difference.
 *
 * hfa_fa_frame_loss (one wave per frame row; honours hfa_set_grid_cap; label_smoothing is a double so that the frame
 * targets are f32(ls) and f32(1 - ls), the reference's float one-hot clamped by Python floats): terms [B,Tmax,3] f32 = the weighted frame,
 * edge and edge-difference (pair t, t+1; t + 1 < T[b]) loss of frame t, zeros where not taking part; bins [B,Tmax,5]
 * i32 = frame GD bin, edge GD bin, edge label bin, difference GD bin, difference label bin, -1 where not counted.
 * grad (may be NULL; frame (b,t) at grad + b*g_bs + t*g_ld): column 0 and columns 2..V+1 receive
 * coef[0] d frame + coef[1] d edge + coef[3] d difference (+ coef[2] sigmoid'(x) emd_fac[b,t] with emd_fac, from
 * hfa_fa_emd) of the SUMS of the terms, zeros where not taking part; coef [4] f32 on the device = upstream gradient /
 * normaliser per loss (x 1/2 for the EMD), so a backward pass needs no host synchronisation.
 *
 * hfa_fa_emd (one workgroup per row): forward and reverse inclusive scans of d_t = sigmoid(x_t) - ph_edge_t over
 * t < T[b] in f64.  sums [B,3] f64 = sum_{u<T} |F_u|, sum_u |R_u| and |sum d| (each of the Tmax - T[b] padding columns
 * adds the last to the first, which hfa_fa_loss_reduce does in closed form; for u >= T[b] R_u is 0); fac [B,Tmax] i32 = sum_{u>=t} sign(F_u) + sum_{u<=t} sign(R_u), padding included (exact
 * integer counts), zeros where not taking part.
 *
 * hfa_fa_loss_reduce (one workgroup per row over a fixed tree on the frame index, then the rows in ascending order;
 * honours hfa_set_grid_cap): row_terms [B,4] f64 = each row's unnormalised sums (EMD: (sums[b,0] + (Tmax - T[b]) sums[b,2] + sums[b,1]) / 2),
 * the same bits alone and in a batch; hist as above (integer atomics); norm [4] f64 = live frames, frames, full rows x
 * Tmax, pairs; losses [4] f64 = sum_b row_terms / norm (0 where norm is 0). */
int hfa_fa_frame_loss(int B, int Tmax, int V, int num_bins, double label_smoothing, const int32_t* T,
                      const int32_t* label_type, const float* logits, long long ld, long long bs,
                      const int32_t* ph_frame, const float* ph_edge, const int32_t* ph_mask, const float* tables,
                      float* terms, int32_t* bins, const float* coef, const int32_t* emd_fac, float* grad,
                      long long g_ld, long long g_bs, hipStream_t stream);
int hfa_fa_emd(int B, int Tmax, const int32_t* T, const int32_t* label_type, const float* logits, long long ld,
               long long bs, const float* ph_edge, double* sums, int32_t* fac, hipStream_t stream);
int hfa_fa_loss_reduce(int B, int Tmax, int V, int num_bins, const int32_t* T, const int32_t* label_type,
                       const float* terms, const int32_t* bins, const int32_t* ph_frame, const double* emd_sums,
                       double* row_terms, double* losses, double* norm, int32_t* hist, hipStream_t stream);

/* ---- head fine-tuning (hubertfa_amd/csrc/train.hip) ------------------------------------------------------------------
 * What a training step of the head alone needs after the losses' d loss / d logits: the backbone frozen
 * as optimizer_config.freeze allows (networks/task/forced_alignment.py:499-501) under a new or continued nn.Linear head
 * (load_pretrained, forced_alignment.py:118-125).  Conventions of the CTC block.
 *
 * hfa_wgrad_f32 replaces autograd's backward of the head's nn.Linear (forced_alignment.py:53-55) with respect to its
 * weight and bias, over a variable-length batch:
 *   dW[n*ldw + c] = sum_b sum_{t < lens[b]} G[b,t,n] X[b,t,c],  db[n] = sum_b sum_{t < lens[b]} G[b,t,n]  (n < N, c < C),
 *   *sumsq (f64) = sum dW^2 + sum db^2 of the f32 values written (torch.nn.utils.clip_grad_norm_'s total norm, squared).
 * G row (b,t) at G + b*g_bs + t*ldg (N floats, ldg >= N), X row (b,t) at X + b*x_bs + t*ldx (C floats, ldx >= C), lens [B]
 * i32 on the device (clamped to 0..Tmax); rows t >= lens[b] and columns past N / C are never loaded, so nothing there
 * (NaN included) reaches a result; lens[b] = 0 is legal; every element of dW [N][C] (ldw >= C), db [N] and sumsq is
 * written (zeros when no row is live).  N >= 1, C a positive multiple of 8.  The f32 MFMA (v_mfma_f32_16x16x4_f32), not
 * the split-f16 scheme: G carries the losses' 1 / sum T normalisers, i.e. f16 subnormals.  The reduction is cut into
 * chunks of hfa_wgrad_chunk_rows() = 256 rows of one batch row, chunk (b, t / 256) whatever the grid; each chunk's f32
 * partial of dW (a chain over its rows in ascending t) and f64 partial of db go to the workspace (hfa_wgrad_workspace_bytes(B, Tmax, N, C) bytes,
 * 8-byte aligned, the caller's), a second pass adds the live chunks in ascending order in f64 and a third the squares in
 * a fixed order: no float atomics, the same bits on every run and under hfa_set_grid_cap (which the first two passes
 * honour).  Three launches, no allocation, no synchronisation.
 *
 * hfa_adamw_f32: one launch over the flat f32 buffers p, m (exp_avg), v (exp_avg_sq), g [n]: first the norm clip of
 * torch.nn.utils.clip_grad_norm_ (the trainer's gradient_clip_val, train.py:139-141), g' = f32(g * f32(min(1, max_norm /
 * (sqrt(*sumsq) + 1e-6)))) (max_norm <= 0: no clipping; g itself is not written), then one torch.optim.AdamW step
 * (forced_alignment.py:473-486; amsgrad off): p *= 1 - lr wd; m = beta1 m + (1 - beta1) g'; v = beta2 v + (1 - beta2) g'^2;
 * p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps), each element in f64 from the f32 state and rounded once.  bc1 = 1 -
 * beta1^step and bc2 = 1 - beta2^step come from the host, which knows the step (with OneCycleLR's cycle_momentum,
 * forced_alignment.py:487-497, beta1 is the step's own); sumsq is the device scalar hfa_wgrad_f32 wrote, so nothing makes
 * the host wait.  Deviation from the reference: when *sumsq is not finite the step is skipped -- p, m and v keep their
 * bits and *skipped (i32, device) is incremented -- where clip_grad_norm_ would write NaN into every weight. */
long long hfa_wgrad_workspace_bytes(int B, int Tmax, int N, int C);
int hfa_wgrad_chunk_rows(void);
int hfa_wgrad_f32(int B, int Tmax, int N, int C, const float* G, long long ldg, long long g_bs, const float* X,
                  long long ldx, long long x_bs, const int32_t* lens, float* dW, long long ldw, float* db,
                  double* sumsq, void* workspace, hipStream_t stream);
int hfa_adamw_f32(long long n, float* p, float* m, float* v, const float* g, const double* sumsq, double max_norm,
                  double lr, double beta1, double beta2, double eps, double weight_decay, double bc1, double bc2,
                  int32_t* skipped, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* HFA_H_ */
