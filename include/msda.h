/*
 * msda.h — C ABI of libmsda_hip.so: multi-scale deformable attention
 * forward / backward for AMD MI355X (gfx950), hand-written HIP.
 *
 * This is the drop-in boundary for the reference's native op.  Each entry point
 * replaces one function of the reference's pybind module
 * `MultiScaleDeformableAttention` (paths relative to the UVHand repo):
 *
 *   msda_forward_*   <-  ms_deform_attn_forward   models/ops/src/vision.cpp:14,
 *                        models/ops/src/ms_deform_attn.h:20-39, which dispatches to
 *                        ms_deform_attn_cuda_forward  models/ops/src/cuda/ms_deform_attn_cuda.cu:20-80
 *                        (kernel: models/ops/src/cuda/ms_deform_im2col_cuda.cuh:237-299)
 *   msda_backward_*  <-  ms_deform_attn_backward  models/ops/src/vision.cpp:15,
 *                        models/ops/src/ms_deform_attn.h:42-61, which dispatches to
 *                        ms_deform_attn_cuda_backward models/ops/src/cuda/ms_deform_attn_cuda.cu:83-153
 *                        (kernels: models/ops/src/cuda/ms_deform_im2col_cuda.cuh:301-920)
 *
 * The reference passes at::Tensor; this ABI passes what those tensors are: raw
 * DEVICE pointers into caller-owned, contiguous, row-major storage plus sizes:
 *
 *   value          [N, S, M, D]           T      S = sum_l H_l*W_l
 *   spatial_shapes [L, 2]  (H_l, W_l)     int64  device memory (read in-kernel, as the
 *   level_start    [L]                    int64  reference does: im2col_cuda.cuh:274-277)
 *   sampling_loc   [N, Lq, M, L, P, 2]    TL     (x, y), normalised to the level's extent
 *   attn_weight    [N, Lq, M, L, P]       TL
 *   out / grad_out [N, Lq, M*D]           T
 *   grad_value     [N, S, M, D]           T
 *   grad_sampling_loc, grad_attn_weight   TL     same shapes as sampling_loc / attn_weight
 *
 *   suffix  T        TL      accumulation
 *   f32     float    float   float            (the reference's float instantiation)
 *   f64     double   double  double           (the reference's double instantiation; gradcheck)
 *   bf16    bf16     float   float            (new capability, no reference counterpart: bf16 storage
 *                                              of the value-like tensors, D = 32 family only)
 *
 * Semantics kept from the reference: the batch is processed whole (im2col_step
 * only chunks the reference's launches; results do not depend on it, the host
 * wrapper validates it); every output element is written by the call — the
 * caller does NOT need to zero out / grad_* beforehand (the reference zero-fills
 * them on the host side, ms_deform_attn_cuda.cu:54,121-123).
 *
 * Ownership: the library allocates nothing and frees nothing, reads no environment
 * variable, and keeps no process-wide mutable state that any computation depends on: the error string and
 * the test hook msda_force_path() are per thread (msda_launch_count() is a diagnostic counter).  It never synchronises the
 * device: all work (including the zero-fill of grad_value where a kernel needs
 * it) is enqueued on `stream` (a hipStream_t; NULL = the default stream).
 * Re-entrant: forward and backward may be called concurrently from different
 * host threads (the backward arrives on PyTorch's autograd thread).
 *
 * Alignment: tensors obtained from an allocator always qualify.  The D = 32 kernels move rows as 16-byte
 * (fp32) / 8-byte (bf16) vectors and (x, y) pairs as 8 bytes; an fp32 call whose tensors are only
 * element-aligned (a contiguous view at an odd offset) is served by the generic kernels, the bf16,
 * fused-prologue and weight-gradient entry points return MSDA_ERR_ARGUMENT for such pointers.
 *
 * Errors: every function returns 0 on success, non-zero on failure, in which
 * case msda_last_error() describes it.  Unlike the reference, which only
 * printf()s a failed launch (im2col_cuda.cuh:948-952, 1321-1325), launch errors
 * are returned.
 */
#ifndef MSDA_H_
#define MSDA_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSDA_OK            0
#define MSDA_ERR_ARGUMENT  1   /* null pointer, non-positive size, index range beyond int32 */
#define MSDA_ERR_LAUNCH    2   /* HIP runtime reported an error at enqueue time */

/* Which kernel family a call would use for the given geometry (for tests/bench):
 * 0 = generic (any D, any dtype), 1 = D=32 fast path. */
#define MSDA_PATH_GENERIC  0
#define MSDA_PATH_D32      1

typedef void *msda_stream_t; /* hipStream_t */

int msda_forward_f32(const float *value, const int64_t *spatial_shapes, const int64_t *level_start,
                     const float *sampling_loc, const float *attn_weight,
                     int N, int S, int M, int D, int L, int Lq, int P,
                     float *out, msda_stream_t stream);

int msda_backward_f32(const float *grad_out, const float *value, const int64_t *spatial_shapes,
                      const int64_t *level_start, const float *sampling_loc, const float *attn_weight,
                      int N, int S, int M, int D, int L, int Lq, int P,
                      float *grad_value, float *grad_sampling_loc, float *grad_attn_weight,
                      msda_stream_t stream);

int msda_forward_f64(const double *value, const int64_t *spatial_shapes, const int64_t *level_start,
                     const double *sampling_loc, const double *attn_weight,
                     int N, int S, int M, int D, int L, int Lq, int P,
                     double *out, msda_stream_t stream);

int msda_backward_f64(const double *grad_out, const double *value, const int64_t *spatial_shapes,
                      const int64_t *level_start, const double *sampling_loc, const double *attn_weight,
                      int N, int S, int M, int D, int L, int Lq, int P,
                      double *grad_value, double *grad_sampling_loc, double *grad_attn_weight,
                      msda_stream_t stream);

/* bf16 tensors are passed as uint16_t* (raw bfloat16 bits); all arithmetic and accumulation is fp32, one rounding at
 * the final store.  D = 32 geometries take the tiled kernels, every other D (or rows at an odd element offset) the
 * generic ones.  msda_backward_bf16 (bf16 grad_value) exists for the D = 32 family only and returns MSDA_ERR_ARGUMENT
 * elsewhere — msda_backward_bf16_gv32 below serves every geometry (msda_path_for(2, M, D, L, P) tells which is which). */
int msda_forward_bf16(const uint16_t *value, const int64_t *spatial_shapes, const int64_t *level_start,
                      const float *sampling_loc, const float *attn_weight,
                      int N, int S, int M, int D, int L, int Lq, int P,
                      uint16_t *out, msda_stream_t stream);

int msda_backward_bf16(const uint16_t *grad_out, const uint16_t *value, const int64_t *spatial_shapes,
                       const int64_t *level_start, const float *sampling_loc, const float *attn_weight,
                       int N, int S, int M, int D, int L, int Lq, int P,
                       uint16_t *grad_value, float *grad_sampling_loc, float *grad_attn_weight,
                       msda_stream_t stream);

/* bf16 rows in, fp32 grad_value out.  Same as msda_backward_bf16 except that grad_value is float[N,S,M,D]:
 * nothing is rounded between the query chunks ("passes") of a long backward, which also lets those passes
 * accumulate in place in global memory instead of in an LDS tile (cfg-4 encoder regime: 2x faster than
 * msda_backward_bf16), and a caller whose `value` parameter is fp32 needs no conversion of the result.
 * msda_backward_passes(Lq, P) = number of passes the D = 32 backward takes (1 = single pass). */
int msda_backward_bf16_gv32(const uint16_t *grad_out, const uint16_t *value, const int64_t *spatial_shapes,
                            const int64_t *level_start, const float *sampling_loc, const float *attn_weight,
                            int N, int S, int M, int D, int L, int Lq, int P,
                            float *grad_value, float *grad_sampling_loc, float *grad_attn_weight,
                            msda_stream_t stream);
int msda_backward_passes(int Lq, int P);

/* ---- Backward with flags and caller-provided scratch (D = 32 family) -----------------------------------
 * flags = 0: exactly msda_backward_*.
 * flags & MSDA_FLAG_DETERMINISTIC: grad_value is bitwise reproducible run to run (grad_sampling_loc and
 * grad_attn_weight always are).  The default kernels order the contributions to a pixel by the rank an LDS
 * integer atomic returned, the reference by the arrival of its atomicAdds (ms_deform_im2col_cuda.cuh:125-152);
 * both differ in the last bits between runs.  With the flag the D = 32 kernels run the same sort + gather with one
 * counter per (pixel row, WAVEFRONT) — eight 16-bit counters packed in four LDS words per row — so that a row's
 * records end up wavefront-major in sampling-point order, a pure function of the inputs (uvhand_amd/csrc/
 * msda_d32_value.h, DET), inside the same single launch as the default mode.  It needs no scratch: `workspace` may be NULL
 * (msda_backward_workspace_bytes() says what a call can use; with this flag alone that is nothing).
 * Shapes that are inconsistent with S (a level whose pixels do not lie in [0, S)) never cause an
 * out-of-range access on this path: such a level contributes nothing and pixels no level covers get zeros.
 * Outside the D = 32 family (any D, fp64, element-aligned views) the flag selects a destination-major kernel that
 * adds a pixel's contributions in (query, point) order — no atomics, no scratch, rows x Lq*P point tests of work; a call
 * with N*S*M x Lq*P > 2^36 is refused (MSDA_ERR_ARGUMENT) rather than run for seconds.  A pixel that several levels cover
 * (overlapping level_start ranges: not something the reference's callers produce) is credited to the first such level there,
 * to every level by the default kernels: overlapping levels are unsupported in every deterministic path.
 * Cost on the D = 32 family: 3-15 % over the default backward (profiles/r03_notes.md section 4).  Replaces the same reference functions as msda_backward_*. */
#define MSDA_FLAG_DETERMINISTIC 1u
/* msda_backward_workspace_bytes only: the size is asked for a msda_backward_prologue_* call (on large problems its
 * grad_sampling_loc / grad_attn_weight workgroups see one head each and leave the reference-point gradient per head in
 * the scratch; without scratch the call runs the kernels that need none). */
#define MSDA_FLAG_PROLOGUE 2u
/* the workspace of this backward call STARTS WITH the table a msda_forward_ws_* / msda_forward_prologue_ws_* call of the same
 * geometry filled from the same sampling locations / attention weights (below); any scratch the call uses follows it, at the
 * table's size rounded up to 256 bytes (msda_backward_workspace_bytes with this flag = both).  The table is ignored where the
 * backward's plan reads none (msda_forward_workspace_bytes() == 0, the deterministic flag), where the buffer is too small,
 * or where its stamp says that the forward did not write it. */
#define MSDA_FLAG_FORWARD_TABLE 4u
/* grad_value of EVERY level through the sort + gather kernels, none as a dense product on the matrix cores (large problems,
 * levels of at most 64 pixels: uvhand_amd/csrc/msda_d32_dense.h).  The results agree to fp32 summation order either way while
 * grad_out is finite.  A non-finite grad_out row differs: in the dense product a zero weight still multiplies every query's
 * row (0 x Inf = NaN), so ALL pixels of that (batch, head)'s dense levels become NaN, where the reference's atomicAdd
 * (ms_deform_im2col_cuda.cuh:125-152) — and this flag — poison only the pixels that query's taps land on.  Costs the dense
 * levels' speed-up (cfg-4 encoder backward +8 %); GradScaler-style loops that discard a non-finite step do not need it. */
#define MSDA_FLAG_EXACT_NONFINITE 8u
unsigned long long msda_backward_workspace_bytes(int N, int S, int M, int D, int L, int Lq, int P, unsigned flags);
/* 1 if a backward of this geometry honours MSDA_FLAG_DETERMINISTIC, 0 if it would be refused (MSDA_ERR_ARGUMENT): outside
 * the D = 32 family (elem_bytes 8 = fp64, any D != 32, ...) the deterministic kernel is a brute-force test of every sampling
 * point against every pixel row, bounded at N*S*M x Lq*P <= 2^36.  Hosts that run under
 * torch.use_deterministic_algorithms(True, warn_only=True) ask first, warn, and clear the flag.  Pure host logic. */
int msda_deterministic_supported(int elem_bytes, int N, int S, int M, int D, int L, int Lq, int P);
int msda_backward_ws_f32(const float *grad_out, const float *value, const int64_t *spatial_shapes,
                         const int64_t *level_start, const float *sampling_loc, const float *attn_weight,
                         int N, int S, int M, int D, int L, int Lq, int P,
                         float *grad_value, float *grad_sampling_loc, float *grad_attn_weight,
                         void *workspace, unsigned long long workspace_bytes, unsigned flags, msda_stream_t stream);
int msda_backward_ws_f64(const double *grad_out, const double *value, const int64_t *spatial_shapes,
                         const int64_t *level_start, const double *sampling_loc, const double *attn_weight,
                         int N, int S, int M, int D, int L, int Lq, int P,
                         double *grad_value, double *grad_sampling_loc, double *grad_attn_weight,
                         void *workspace, unsigned long long workspace_bytes, unsigned flags, msda_stream_t stream);
int msda_backward_ws_bf16(const uint16_t *grad_out, const uint16_t *value, const int64_t *spatial_shapes,
                          const int64_t *level_start, const float *sampling_loc, const float *attn_weight,
                          int N, int S, int M, int D, int L, int Lq, int P,
                          uint16_t *grad_value, float *grad_sampling_loc, float *grad_attn_weight,
                          void *workspace, unsigned long long workspace_bytes, unsigned flags, msda_stream_t stream);
int msda_backward_ws_bf16_gv32(const uint16_t *grad_out, const uint16_t *value, const int64_t *spatial_shapes,
                               const int64_t *level_start, const float *sampling_loc, const float *attn_weight,
                               int N, int S, int M, int D, int L, int Lq, int P,
                               float *grad_value, float *grad_sampling_loc, float *grad_attn_weight,
                               void *workspace, unsigned long long workspace_bytes, unsigned flags, msda_stream_t stream);

/* ---- Forward that prepares its backward (D = 32 family) -----------------------------------------------------
 * The reference's backward re-derives every sampling point's geometry from sampling_loc / attn_weight
 * (ms_deform_im2col_cuda.cuh:340-371, inside every one of its 32 channel threads).  Here the FORWARD already computes it once
 * per point; msda_forward_ws_* additionally leaves in `workspace` what the backward of the same autograd node would otherwise
 * work out again (pass the same buffer as `workspace` with MSDA_FLAG_FORWARD_TABLE to msda_backward_ws_*; for the
 * fused-prologue pair: msda_forward_prologue_ws_* and msda_backward_prologue_ws_f32 / _bf16_gv32):
 *   small problems (every workgroup of the backward launch resident at once — the 300-query decoder shape): a level-major
 *     POINT TABLE, 16 bytes per sampling point, entry ((b*M + m)*L + l) * Lq*P + q*P + p = {tap validity bits << 24 | pixel
 *     index of the top-left tap + W + 1, the two bilinear fractions, the attention weight}, and behind it a header with the
 *     pixel range of every grad_value workgroup;
 *   large problems whose grad_value pass cuts the levels into W <= 8 pixel ranges (the encoder shapes): RANGE MASKS, one
 *     byte per sampling point, level-major — bit t set iff a tap of the point may land in range t — which turn every range's
 *     strided scan of sampling_loc into a coalesced byte scan.
 * grad_sampling_loc and grad_attn_weight are bit-identical with and without the buffer; grad_value is equal up to the order
 * in which a pixel's contributions are summed (as between any two runs of the default kernels).  Each buffer carries a stamp
 * that the forward writes and the backward checks: a forward call that cannot fill the buffer (rows that are not 16-byte
 * aligned take the generic kernels) clears it, and the backward then ignores the buffer.
 * msda_forward_workspace_bytes(): the buffer's size for a geometry, 0 where the backward's plan reads none; flags:
 * MSDA_FLAG_PROLOGUE for the fused-prologue pair.  workspace NULL / too small / unaligned (16 bytes): exactly msda_forward_*.
 * The caller owns the buffer and keeps it, unmodified, with the tensors it saves for the backward. */
unsigned long long msda_forward_workspace_bytes(int N, int S, int M, int D, int L, int Lq, int P, unsigned flags);
int msda_forward_ws_f32(const float *value, const int64_t *spatial_shapes, const int64_t *level_start,
                        const float *sampling_loc, const float *attn_weight,
                        int N, int S, int M, int D, int L, int Lq, int P,
                        float *out, void *workspace, unsigned long long workspace_bytes, msda_stream_t stream);
int msda_forward_ws_bf16(const uint16_t *value, const int64_t *spatial_shapes, const int64_t *level_start,
                         const float *sampling_loc, const float *attn_weight,
                         int N, int S, int M, int D, int L, int Lq, int P,
                         uint16_t *out, void *workspace, unsigned long long workspace_bytes, msda_stream_t stream);

/* ---- Fused module prologue (fp32, D = 32 family) ---------------------------------
 * The module computes  attn = softmax(logits) over the L*P points of a (query, head)  and
 * sampling_loc = reference_point + offset / (W_l, H_l)  (models/ops/modules/ms_deform_attn.py:101-108,
 * :110-128 after the 21-keypoint mean) with elementwise PyTorch kernels before calling the op.  These
 * entry points take the RAW tensors instead and do that arithmetic in the kernels' point lanes:
 *   forward : reference_points[N,Lq,L,2], sampling_offsets[N,Lq,M,L,P,2] (pixels), attn_logits[N,Lq,M,L*P]
 *             -> out, plus sampling_loc_out / attn_weight_out (what the unfused path would have been
 *             given; saved for the backward)
 *   backward: takes those saved tensors; returns grad_value and the gradients of the RAW tensors
 *             (offsets, logits — softmax backward included — and reference points, summed over heads
 *             and points).
 * The module produces offsets and logits with two nn.Linear layers on the same input (:100-101); run as
 * ONE GEMM their outputs are column blocks of a [N*Lq, ld] matrix.  ld_offsets / ld_logits are the floats
 * between consecutive (batch, query) rows of those two tensors (0 = dense: 2*M*L*P and M*L*P); the raw
 * gradients are written with ld_grad_offsets / ld_grad_logits the same way, so the backward of that one
 * GEMM reads them in place.  Offsets need an even stride and an 8-byte aligned base.
 * msda_prologue_supported() != 0 iff the geometry qualifies (D = 32 family, L*P and P powers of two,
 * whole queries per workgroup); otherwise callers compose the plain entry points as the reference does. */
int msda_prologue_supported(int N, int S, int M, int D, int L, int Lq, int P);
int msda_forward_prologue_f32(const float *value, const int64_t *spatial_shapes, const int64_t *level_start,
                              const float *reference_points, const float *sampling_offsets, const float *attn_logits,
                              int N, int S, int M, int D, int L, int Lq, int P, long long ld_offsets, long long ld_logits,
                              float *out, float *sampling_loc_out, float *attn_weight_out, msda_stream_t stream);
int msda_backward_prologue_f32(const float *grad_out, const float *value, const int64_t *spatial_shapes,
                               const int64_t *level_start, const float *sampling_loc, const float *attn_weight,
                               int N, int S, int M, int D, int L, int Lq, int P, long long ld_grad_offsets,
                               long long ld_grad_logits, float *grad_value, float *grad_sampling_offsets,
                               float *grad_attn_logits, float *grad_reference_points, msda_stream_t stream);
/* msda_forward_prologue_f32 that also leaves the point table (msda_forward_workspace_bytes(..., MSDA_FLAG_PROLOGUE)) */
int msda_forward_prologue_ws_f32(const float *value, const int64_t *spatial_shapes, const int64_t *level_start,
                                 const float *reference_points, const float *sampling_offsets, const float *attn_logits,
                                 int N, int S, int M, int D, int L, int Lq, int P, long long ld_offsets, long long ld_logits,
                                 float *out, float *sampling_loc_out, float *attn_weight_out, void *workspace,
                                 unsigned long long workspace_bytes, msda_stream_t stream);
/* same with flags / scratch (MSDA_FLAG_DETERMINISTIC, MSDA_FLAG_FORWARD_TABLE, msda_backward_workspace_bytes) */
int msda_backward_prologue_ws_f32(const float *grad_out, const float *value, const int64_t *spatial_shapes,
                                  const int64_t *level_start, const float *sampling_loc, const float *attn_weight,
                                  int N, int S, int M, int D, int L, int Lq, int P, long long ld_grad_offsets,
                                  long long ld_grad_logits, float *grad_value, float *grad_sampling_offsets,
                                  float *grad_attn_logits, float *grad_reference_points, void *workspace,
                                  unsigned long long workspace_bytes, unsigned flags, msda_stream_t stream);

/* bf16 rows through the fused prologue (value / out / grad_out in bf16; offsets, logits, reference points and EVERY
 * gradient in fp32 — grad_value too: its passes accumulate in fp32 and a caller whose value_proj runs in fp32 wants it so).
 * Same geometry rule (msda_prologue_supported), same row strides, same flags / workspace as the f32 entry points. */
int msda_forward_prologue_bf16(const uint16_t *value, const int64_t *spatial_shapes, const int64_t *level_start,
                               const float *reference_points, const float *sampling_offsets, const float *attn_logits,
                               int N, int S, int M, int D, int L, int Lq, int P, long long ld_offsets, long long ld_logits,
                               uint16_t *out, float *sampling_loc_out, float *attn_weight_out, msda_stream_t stream);
int msda_forward_prologue_ws_bf16(const uint16_t *value, const int64_t *spatial_shapes, const int64_t *level_start,
                                  const float *reference_points, const float *sampling_offsets, const float *attn_logits,
                                  int N, int S, int M, int D, int L, int Lq, int P, long long ld_offsets, long long ld_logits,
                                  uint16_t *out, float *sampling_loc_out, float *attn_weight_out, void *workspace,
                                  unsigned long long workspace_bytes, msda_stream_t stream);
int msda_backward_prologue_bf16_gv32(const uint16_t *grad_out, const uint16_t *value, const int64_t *spatial_shapes,
                                     const int64_t *level_start, const float *sampling_loc, const float *attn_weight,
                                     int N, int S, int M, int D, int L, int Lq, int P, long long ld_grad_offsets,
                                     long long ld_grad_logits, float *grad_value, float *grad_sampling_offsets,
                                     float *grad_attn_logits, float *grad_reference_points, void *workspace,
                                     unsigned long long workspace_bytes, unsigned flags, msda_stream_t stream);

/* ---- Bracketing projections ----------------------------------------------------
 * Weight and bias gradient of an fp32 nn.Linear  y[M,N] = x[M,K] . W[N,K]^T + b[N]:
 *     grad_weight[N,K] = grad_out[M,N]^T . input[M,K]        grad_bias[N] = sum_m grad_out[m,:]
 * i.e. the GEMM autograd issues for value_proj / sampling_offsets / attention_weights / output_proj
 * (models/ops/modules/ms_deform_attn.py:96,100,101,139), as a split-M fp32-MFMA kernel with a
 * fixed-order reduction (bitwise reproducible).  N and K must be multiples of 4; grad_bias may be
 * NULL; `workspace` must hold msda_linear_wgrad_workspace_bytes(M, N, K) bytes (may be 0 -> NULL ok).
 * The forward GEMM and the input gradient: msda_linear_forward_f32 / msda_linear_dgrad_f32 below. */
unsigned long long msda_linear_wgrad_workspace_bytes(int M, int N, int K);
int msda_linear_wgrad_f32(const float *grad_out, const float *input, int M, int N, int K,
                          float *grad_weight, float *grad_bias, void *workspace, msda_stream_t stream);

/* Padding mask of value_proj (models/ops/modules/ms_deform_attn.py:97-98:
 * value = value.masked_fill(input_padding_mask[..., None], 0)) without the two full passes over
 * [N, S, C] that masked_fill and its backward cost:
 *   msda_zero_masked_rows_f32     x[r, :] = 0 where row_mask[r] != 0, in place (forward: on the GEMM output;
 *                                 backward: on the input gradient) — touches the mask and the masked rows only;
 *   msda_linear_wgrad_masked_f32  msda_linear_wgrad_f32 with the rows of grad_out where row_mask[r] != 0
 *                                 taken as zero (row_mask may be NULL = no mask).
 * row_mask: one byte per row (a torch.bool tensor's storage).  cols must be a multiple of 4, x 16-byte aligned. */
int msda_linear_wgrad_masked_f32(const float *grad_out, const float *input, const uint8_t *row_mask, int M, int N, int K,
                                 float *grad_weight, float *grad_bias, void *workspace, msda_stream_t stream);
/* bf16 operands (what the layer sees under torch.autocast(bfloat16)), fp32 products, accumulation and results: the weight
 * gradient reaches the fp32 master parameter without a rounding to bf16 in between, at half the operand bytes.  Same
 * workspace size as the f32 entry point; grad_out / input 8-byte aligned. */
int msda_linear_wgrad_masked_bf16(const uint16_t *grad_out, const uint16_t *input, const uint8_t *row_mask, int M, int N, int K,
                                  float *grad_weight, float *grad_bias, void *workspace, msda_stream_t stream);
/* `count` (1..4) weight gradients in one call: the first stages one after the other, then ONE fixed-order second stage for
 * all of them (the module's backward has three: output_proj, the merged projection, value_proj — at decoder sizes the three
 * separate second stages cost as much as a first stage).  Host arrays of `count` entries; row_mask / grad_bias may be NULL
 * (array) or hold NULL entries; workspace[p] as for msda_linear_wgrad_f32 with that problem's sizes.  Results are bitwise
 * those of `count` msda_linear_wgrad_masked_{f32,bf16} calls.
 *   msda_linear_wgrad_multi      operands fp32 or bf16 PER PROBLEM: operands_bf16[p] != 0 -> grad_out[p] / input[p] are bf16
 *                                (uint16_t), as under autocast, where the merged projection stays fp32 and the other two are bf16;
 *                                operands_bf16 == NULL: all fp32;
 *   msda_linear_wgrad_multi_f32  the all-fp32 spelling. */
int msda_linear_wgrad_multi(int count, const void *const *grad_out, const void *const *input, const int *operands_bf16,
                            const uint8_t *const *row_mask, const int *M, const int *N, const int *K, float *const *grad_weight,
                            float *const *grad_bias, void *const *workspace, msda_stream_t stream);
int msda_linear_wgrad_multi_f32(int count, const float *const *grad_out, const float *const *input, const uint8_t *const *row_mask,
                                const int *M, const int *N, const int *K, float *const *grad_weight, float *const *grad_bias,
                                void *const *workspace, msda_stream_t stream);
int msda_zero_masked_rows_f32(float *x, const uint8_t *row_mask, long long rows, int cols, msda_stream_t stream);
/* Up to four fp32 -> bf16 conversions (round to nearest even) in ONE launch: the weights and biases of value_proj / output_proj
 * that torch.autocast(bfloat16) casts on every call (models/ops/modules/ms_deform_attn.py:96,139 under the reference's --amp) —
 * four ~3 us kernels otherwise.  src / dst / n: host arrays of `count` (1..4) device pointers and element counts (each a
 * multiple of 2; sources 8-byte, destinations 4-byte aligned). */
int msda_cast_bf16_multi_f32(int count, const float *const *src, uint16_t *const *dst, const long long *n, msda_stream_t stream);

/* Forward and input gradient of the same fp32 layers (nn.Linear semantics, models/ops/modules/ms_deform_attn.py:96,100,101,139
 * and what autograd derives for them):
 *     output[rows, out]    = input[rows, in] . weight[out, in]^T + bias[out]        (bias may be NULL)
 *     grad_input[rows, in] = grad_out[rows, out] . weight[out, in]
 * as one plain fp32-MFMA launch each (exact fp32 products, fixed summation order: bitwise reproducible) — at this module's
 * shapes the vendor BLAS path costs more on the host (~27 us per GEMM through torch) than these kernels run for.  row_mask
 * (may be NULL; one byte per row): rows with a non-zero byte are WRITTEN AS ZEROS — value.masked_fill(padding_mask, 0) after
 * value_proj (modules/ms_deform_attn.py:97-98) and its backward, without a second pass.  out_features and in_features must
 * be multiples of 4, all operands 16-byte aligned and contiguous. */
int msda_linear_forward_f32(const float *input, const float *weight, const float *bias, const uint8_t *row_mask, long long rows,
                            int out_features, int in_features, float *output, msda_stream_t stream);
int msda_linear_dgrad_f32(const float *grad_out, const float *weight, const uint8_t *row_mask, long long rows, int out_features,
                          int in_features, float *grad_input, msda_stream_t stream);

/* Thread-local description of the last failure on the calling thread ("" if none). */
/* ---- Residual add + LayerNorm of the layers around the op --------------------------
 * y = LayerNorm(x + residual) * gamma + beta over rows of width d (fp32, d a multiple of 4, <= 1024) — the
 * `x = x + dropout(x2); x = norm(x)` pairs of the reference's encoder / decoder layers
 * (models/arctic_transformer.py:279-282, 294-295, 366-368, 377-378, 385-386) as one pass instead of an add kernel
 * and a LayerNorm kernel; `residual` may be NULL (plain LayerNorm).  The forward also returns mean[rows] and
 * rstd[rows]; the backward recomputes x + residual, writes grad_sum[rows, d] (the gradient of x and of residual
 * alike) and grad_gamma / grad_beta through per-workgroup partial sums in `workspace`
 * (msda_add_layernorm_workspace_bytes) combined in a fixed order — reproducible, no float atomics.  Dropout is not
 * part of it: the caller applies the framework's dropout to `residual` first, so its random stream is untouched. */
unsigned long long msda_add_layernorm_workspace_bytes(long long rows, int d);
int msda_add_layernorm_forward_f32(const float *x, const float *residual, const float *gamma, const float *beta, long long rows,
                                   int d, float eps, float *y, float *mean, float *rstd, msda_stream_t stream);
int msda_add_layernorm_backward_f32(const float *grad_y, const float *x, const float *residual, const float *gamma,
                                    const float *mean, const float *rstd, long long rows, int d, float *grad_sum,
                                    float *grad_gamma, float *grad_beta, void *workspace, msda_stream_t stream);
/* The same with a bf16 `residual` (required, rows 8-byte aligned) next to the fp32 x: what the layers pass under
 * bf16 autocast (x the fp32 residual stream, residual the dropout of a bf16 projection output).  The residual is widened
 * exactly on load and the arithmetic is the fp32 entries'; the backward writes grad_x (fp32) and, in the same pass, the same
 * values rounded to bf16 into grad_residual (8-byte aligned). */
int msda_add_layernorm_forward_f32_bf16res(const float *x, const uint16_t *residual, const float *gamma, const float *beta,
                                           long long rows, int d, float eps, float *y, float *mean, float *rstd, msda_stream_t stream);
int msda_add_layernorm_backward_f32_bf16res(const float *grad_y, const float *x, const uint16_t *residual, const float *gamma,
                                            const float *mean, const float *rstd, long long rows, int d, float *grad_x,
                                            uint16_t *grad_residual, float *grad_gamma, float *grad_beta, void *workspace,
                                            msda_stream_t stream);

/* ---- FFN of the layers (models/arctic_transformer.py:283-287, :366-370) ---------------------------
 * linear2(dropout(relu(linear1(x)))): with act = dropout(relu(h)) — the tensor linear2 consumed, saved for its weight gradient
 * anyway — the gradient with respect to h is grad * scale * (act > 0), scale = 1 / (1 - p): one in-place pass over
 * `grad` [n floats, n a multiple of 4, both pointers 16-byte aligned] instead of PyTorch's masked_scale + threshold_backward,
 * and neither the dropout mask nor relu's output has to be kept. */
int msda_relu_dropout_backward_f32(float *grad, const float *act, float scale, long long n, msda_stream_t stream);

/* ---- Decoder self-attention core (models/arctic_transformer.py:351,374-376) -------------------------------
 * nn.MultiheadAttention over the 300 queries (8 heads of 32, batch = frames) computes, between its in- and out-projections,
 *     out = dropout(softmax(q k^T * scale), p) v          for N*H independent (batch, head) problems.
 * These entry points are that core for head_dim 32, fp32, 1 <= Lq, Lk <= 320 (msda_attn32_supported), with neither the
 * [N*H, Lq, Lk] score tensor nor a dropout mask in memory: the forward keeps log-sum-exp per (batch, head, query) [N*H, Lq],
 * the backward (two launches: dK/dV, dQ) recomputes the probabilities and the mask from it.
 * Tensors are views with the head's 32 channels contiguous: element (n, h, l, d) at p + n*sn + h*32 + l*sl + d (strides in
 * floats, multiples of 4; 16-byte aligned bases) — the column blocks of a packed in-projection output [L, N, 3E] are such views.
 * Dropout: keep(seed, pair, query, key) is an integer hash compared with p * 2^32 — the kernel's own random stream.  `seed` is a
 * DEVICE pointer to one 64-bit value (drawn by the caller with its generator; the same value must reach the backward); NULL is
 * allowed when dropout_p == 0.  No attention mask / key-padding mask (the reference's ARCTIC decoder passes none; the masked,
 * long-sequence form is msda_attn32x_* below). */
int msda_attn32_supported(int Lq, int Lk, int head_dim);
int msda_attn32_forward_f32(const float *q, long long q_sn, long long q_sl, const float *k, long long k_sn, long long k_sl,
                            const float *v, long long v_sn, long long v_sl, int N, int H, int Lq, int Lk, float scale,
                            float dropout_p, const unsigned long long *seed, float *out, long long o_sn, long long o_sl, float *lse,
                            msda_stream_t stream);
int msda_attn32_backward_f32(const float *q, long long q_sn, long long q_sl, const float *k, long long k_sn, long long k_sl,
                             const float *v, long long v_sn, long long v_sl, const float *out, long long o_sn, long long o_sl,
                             const float *lse, const float *grad_out, long long go_sn, long long go_sl, int N, int H, int Lq, int Lk,
                             float scale, float dropout_p, const unsigned long long *seed, float *grad_q, long long gq_sn,
                             long long gq_sl, float *grad_k, long long gk_sn, long long gk_sl, float *grad_v, long long gv_sn,
                             long long gv_sl, msda_stream_t stream);
/* The same core with bf16 q, k, v, out, grad_out, grad_q, grad_k, grad_v (uint16_t) — what the decoder's self-attention
 * runs under bf16 autocast.  Same views (strides in elements, multiples of 8; 16-byte aligned bases), same geometry
 * (msda_attn32_supported), lse still fp32 [N*H, Lq].  Arithmetic: q k^T accumulated in fp32, softmax / log-sum-exp in fp32,
 * P rounded to bf16 only as the operand of P v (fp32 accumulate), out rounded once; the backward recomputes P from lse and
 * takes delta = rowsum(dO * O) and dP = dO v^T in fp32, rounds dS = P * (dP - delta) to bf16 only as the operand of dQ and
 * dK, and rounds dQ, dK, dV once.  Dropout: the fp32 entries' hash and threshold — for one seed the two cores drop the same
 * (pair, query, key) entries.  No float atomics: the backward is bitwise reproducible.  At most 53.8 KB of LDS per workgroup. */
int msda_attn32_forward_bf16(const uint16_t *q, long long q_sn, long long q_sl, const uint16_t *k, long long k_sn, long long k_sl,
                             const uint16_t *v, long long v_sn, long long v_sl, int N, int H, int Lq, int Lk, float scale,
                             float dropout_p, const unsigned long long *seed, uint16_t *out, long long o_sn, long long o_sl,
                             float *lse, msda_stream_t stream);
int msda_attn32_backward_bf16(const uint16_t *q, long long q_sn, long long q_sl, const uint16_t *k, long long k_sn, long long k_sl,
                              const uint16_t *v, long long v_sn, long long v_sl, const uint16_t *out, long long o_sn, long long o_sl,
                              const float *lse, const uint16_t *grad_out, long long go_sn, long long go_sl, int N, int H, int Lq,
                              int Lk, float scale, float dropout_p, const unsigned long long *seed, uint16_t *grad_q,
                              long long gq_sn, long long gq_sl, uint16_t *grad_k, long long gk_sn, long long gk_sl,
                              uint16_t *grad_v, long long gv_sn, long long gv_sl, msda_stream_t stream);
/* The masked, long-sequence form of the fp32 core (the DINO decoder: models/dino/deformable_transformer.py:966 runs the
 * module over pad_size + num_queries rows, about 200 + 900, under the contrastive-denoising mask of
 * models/dino/dn_components.py:125-137):
 *     out = dropout(softmax(q k^T * scale + M), p) v,   head_dim 32, fp32, any 1 <= Lq, Lk <= 2048 (msda_attn32x_supported).
 * Views, lse [N*H, Lq] (natural log), seed and the dropout hash are those of msda_attn32_*_f32: for one seed the two cores drop
 * the same (pair, query, key) entries.  Neither operand is resident in LDS as a whole: the forward and dQ own 128 queries per
 * workgroup and stream the keys in chunks of 64 (online softmax in the forward), dK / dV owns 128 keys and streams the queries;
 * ceil(L / 128) workgroups per (batch, head) pair, 18 KB of LDS each.  The backward is two launches (dK / dV, dQ) and forms
 * delta = rowsum(dO * O) itself.  No float atomics, fixed summation order: bitwise reproducible.  No host sync, no allocation.
 * mask: DEVICE bytes [Lq, Lk], row stride mask_sq >= Lk, elements contiguous, shared by every batch entry and head (torch's 2-D
 * boolean attn_mask); nonzero = the key is not visible (M = -inf), zero = visible (M = 0); NULL = no mask.  A hidden entry's
 * probability and dS are exactly 0 in the backward.  A query whose every key is hidden: its out row is NaN (as the module's),
 * its lse -inf, no other row is affected; its gradients are outside the contract (the same mask must reach the backward).
 * Argument errors (lengths, head_dim, misaligned views, p >= 1, p > 0 without a seed, mask_sq < Lk) return MSDA_ERR_ARGUMENT
 * before any launch.  The bf16 form for autocast is msda_attn32x_*_bf16 below. */
int msda_attn32x_supported(int Lq, int Lk, int head_dim);
int msda_attn32x_forward_f32(const float *q, long long q_sn, long long q_sl, const float *k, long long k_sn, long long k_sl,
                             const float *v, long long v_sn, long long v_sl, int N, int H, int Lq, int Lk, float scale,
                             float dropout_p, const unsigned long long *seed, const unsigned char *mask, long long mask_sq,
                             float *out, long long o_sn, long long o_sl, float *lse, msda_stream_t stream);
int msda_attn32x_backward_f32(const float *q, long long q_sn, long long q_sl, const float *k, long long k_sn, long long k_sl,
                              const float *v, long long v_sn, long long v_sl, const float *out, long long o_sn, long long o_sl,
                              const float *lse, const float *grad_out, long long go_sn, long long go_sl, int N, int H, int Lq,
                              int Lk, float scale, float dropout_p, const unsigned long long *seed, const unsigned char *mask,
                              long long mask_sq, float *grad_q, long long gq_sn, long long gq_sl, float *grad_k, long long gk_sn,
                              long long gk_sl, float *grad_v, long long gv_sn, long long gv_sl, msda_stream_t stream);
/* The masked, long-sequence core with bf16 q, k, v, out, grad_out, grad_q, grad_k, grad_v (uint16_t) — what the DINO decoder's
 * self-attention runs under bf16 autocast.  Added after MSDA_ABI_VERSION 116 without a version bump: purely additive.
 * Argument lists, geometry (msda_attn32x_supported), mask, seed, dropout hash, fully-hidden rows and error handling are the
 * _f32 entries'; views as msda_attn32_*_bf16 (strides in elements, multiples of 8; 16-byte aligned bases); lse fp32 [N*H, Lq],
 * natural log.  For one seed all four cores (resident / long, fp32 / bf16) drop the same (pair, query, key) entries.
 * Work split: the forward and dQ own 128 queries per workgroup and stream K and V in chunks of 128 rows, dK / dV owns 128 keys
 * and streams Q and dO (forming the chunk's delta and base-2 lse while loading); 20 KB of LDS (dK / dV 23.5 KB); two backward
 * launches.  Every product on v_mfma_f32_16x16x32_bf16 with fp32 accumulation.  Rounding points (msda_attn32_*_bf16's, carried
 * to the online softmax): scores scaled by scale * log2 e in fp32 after the product; running maximum, running sum and
 * rescaling in fp32; the forward rounds to bf16 only the operand of P v, which is the chunk's UN-NORMALISED, dropout-selected
 * 2^(s - m) — keep_scale / sum is applied once in fp32 at the end and out rounded once (the resident core rounds the normalised
 * P instead: it has the sum before the product).  Backward: P = 2^(s - lse), delta = rowsum(dO * O) from the saved bf16 out in
 * fp32, dP = dO v^T in fp32; P_drop rounded to bf16 as dV's operand, dS = P (dP_drop - delta) rounded to bf16 as dQ's and dK's
 * operand; dQ and dK scaled in fp32, every gradient rounded once.  Hidden and padding entries' P and dS are selected to 0.
 * No atomics, fixed summation order: bitwise reproducible.  No host sync, no allocation; captures in a HIP graph. */
int msda_attn32x_forward_bf16(const uint16_t *q, long long q_sn, long long q_sl, const uint16_t *k, long long k_sn, long long k_sl,
                              const uint16_t *v, long long v_sn, long long v_sl, int N, int H, int Lq, int Lk, float scale,
                              float dropout_p, const unsigned long long *seed, const unsigned char *mask, long long mask_sq,
                              uint16_t *out, long long o_sn, long long o_sl, float *lse, msda_stream_t stream);
int msda_attn32x_backward_bf16(const uint16_t *q, long long q_sn, long long q_sl, const uint16_t *k, long long k_sn, long long k_sl,
                               const uint16_t *v, long long v_sn, long long v_sl, const uint16_t *out, long long o_sn, long long o_sl,
                               const float *lse, const uint16_t *grad_out, long long go_sn, long long go_sl, int N, int H, int Lq,
                               int Lk, float scale, float dropout_p, const unsigned long long *seed, const unsigned char *mask,
                               long long mask_sq, uint16_t *grad_q, long long gq_sn, long long gq_sl, uint16_t *grad_k,
                               long long gk_sn, long long gk_sl, uint16_t *grad_v, long long gv_sn, long long gv_sl,
                               msda_stream_t stream);

/* ---- Transformer input assembly -----------------------------------------------------
 * The flatten block of DeformableTransformer.forward (models/arctic_transformer.py:162-173): per level
 * src_l[N,C,H,W] -> rows [level_start_l, level_start_l + H*W) of src_flatten[N,S,C], and pos_l the same way with
 * level_embed[l][C] added — one tiled-transpose launch for all levels and both tensors instead of the reference's
 * strided torch.cat copies and the add.  `src_levels` / `pos_levels` are HOST arrays of L device pointers, `heights` /
 * `widths` host arrays (the caller knows the feature-map shapes as Python ints; nothing is read back from the device);
 * either tensor family may be NULL.  msda_unflatten_levels_f32 is the inverse copy (the backward: flattened gradient rows
 * back into per-level NCHW gradients, and — with grad_level_embed and a workspace of msda_unflatten_workspace_bytes — the
 * level-embedding gradient as per-tile column sums combined in a fixed order).  fp32, C a multiple of 4, L <= 16. */
int msda_flatten_levels_f32(int L, const float *const *src_levels, const float *const *pos_levels, const float *level_embed,
                            const int *heights, const int *widths, int N, int C, float *src_flatten, float *pos_flatten,
                            msda_stream_t stream);
int msda_unflatten_levels_f32(int L, float *const *grad_src_levels, float *const *grad_pos_levels, const int *heights,
                              const int *widths, int N, int C, const float *grad_src_flatten, const float *grad_pos_flatten,
                              float *grad_level_embed /* [L, C] or NULL */, void *workspace, msda_stream_t stream);
unsigned long long msda_unflatten_workspace_bytes(int L, const int *heights, const int *widths, int N, int C);

const char *msda_last_error(void);

/* ---- Two-stage query selection of the transformer (models/arctic_transformer.py:91-142, :196-232) ----------------------
 * Added after MSDA_ABI_VERSION 116 without a version bump: the five entries below are purely additive (no existing
 * declaration changed), so a binding compiled against 116 keeps working; callers probe them by symbol.
 *
 *   msda_two_stage_proposals_f32  gen_encoder_output_proposals (:106-142), forward: memory [N, S, C] fp32 (C % 4 == 0,
 *       16-byte aligned), padding_mask [N, S] bytes (non-zero = padded), the L levels' heights / widths as HOST int arrays
 *       (S must be their sum of H*W), learnedxy [40] fp32 device or NULL (= 0.05 * 2^lvl).  Writes proposals [N, S, 42]
 *       (logits; +inf at padded rows and rows outside (0.01, 0.99)), memory_out [N, S, C] (memory, those rows zeroed) and
 *       row_mask [N, S] (1 at those rows).  Per level the valid extent is counted on the mask's first column / first row.
 *   msda_two_stage_select_f32     the query selection (:208-232): cls [N, S, K], hand / obj / proposals [N, S, 42]; per frame
 *       the top Q rows by the max class logit, descending (ties: lower row index first; NaN above every number), the class
 *       argmax of each (first maximum; NaN wins) picks the source: hand if it is hand_class0 / hand_class1, object if it
 *       is neither and not 0, the proposal otherwise.  Writes topk [N, Q] int64 (may be NULL), refpoint_unsig [N, Q, 42]
 *       and reference_points = sigmoid(refpoint_unsig) * 2 - 1.  One launch, no synchronisation.  Q > S and
 *       S > 8192 return MSDA_ERR_ARGUMENT; msda_two_stage_select_supported(S, K, Q) tells beforehand (1 = the call runs).
 *   msda_proposal_pos_embed_f32   get_proposal_pos_embed (:91-104): pe [M, 5376] from refpoint_unsig [M, 42];
 *       pe[m, 128c + 2i + s] = s ? cos(u) : sin(u), u = sigmoid(r[m, c]) * 2pi / dim_t[i], dim_t [64] = torch's table at
 *       even indices (:96-97).  pe 16-byte aligned.
 *   msda_proposal_pos_linear_relu_f32  y [M, out] = relu(pe(r) @ weight^T + bias) with weight [out, 5376] (out % 4 == 0,
 *       16-byte aligned), bias [out] or NULL — pos_trans[0:2] without the [M, 5376] table in memory; fp32 MFMA, fixed
 *       summation order. */
int msda_two_stage_proposals_f32(const float *memory, const uint8_t *padding_mask, int N, int S, int C, int L, const int *heights,
                                 const int *widths, const float *learnedxy, float *proposals, float *memory_out, uint8_t *row_mask,
                                 msda_stream_t stream);
int msda_two_stage_select_supported(int S, int K, int Q);
int msda_two_stage_select_f32(const float *cls, const float *hand, const float *obj, const float *proposals, int N, int S, int K,
                              int Q, int hand_class0, int hand_class1, int64_t *topk, float *refpoint_unsig,
                              float *reference_points, msda_stream_t stream);
int msda_proposal_pos_embed_f32(const float *refpoint_unsig, const float *dim_t, long long M, float *pe, msda_stream_t stream);
int msda_proposal_pos_linear_relu_f32(const float *refpoint_unsig, const float *dim_t, const float *weight, const float *bias,
                                      long long M, int out_features, float *y, msda_stream_t stream);

/* ---- The AssemblyHands transformer (models/assembly_transformer.py:23-251, :387-465) ----------------------------------
 * Added after MSDA_ABI_VERSION 116 without a version bump: the three entries below are purely additive (no existing
 * declaration changed), so a binding compiled against 116 keeps working; callers probe them by symbol.
 *
 *   msda_assembly_refine_f32      the decoder's keypoint refinement (:407-465), replacing the boolean-mask add of :442:
 *       reference_points [M, width] (width 2 or 42), cls [M, K] logits, keypoints [M, 63] (21 (x, y, z) triples), all fp32
 *       contiguous; out [M, 42].  hand = argmax(cls) != 0 (first maximum, NaN highest); base = inverse_sigmoid(r) (width 2)
 *       or inverse_sigmoid(((mean of the 21 x, mean of the 21 y) + 0.5) / 2) (width 42), repeated 21 times; hand rows add
 *       each triple's (x, y); out = sigmoid(.) * 2 - 0.5.  inverse_sigmoid: util/misc.py:614-618.  One launch, no sync.
 *   msda_assembly_proposals_f32   gen_encoder_output_proposals (:106-141) for ONE level of H x W rows, as the forward calls
 *       it on the last level (:184): memory points at the level's first row of frame 0, memory_frame_stride (elements, a
 *       multiple of 4) steps frames, C % 4 == 0, 16-byte aligned; padding_mask likewise with mask_frame_stride (bytes).
 *       Writes proposals [N, H*W, 2] (logits; +inf at padded rows and rows outside (0.01, 0.99)), memory_out [N, H*W, C]
 *       (the rows, those zeroed) and row_mask [N, H*W] (1 at those rows).  Valid extent off the mask's first column / row.
 *   msda_assembly_select_f32      the two-stage selection (:202-226), replacing the boolean-mask loop of :204-207: cls
 *       [N, S, K], hand / obj [N, S, 63].  Per frame: object row = the reference's loop (best 0, row 0; for classes
 *       obj_first..obj_last in order, torch.max over rows, update on best < score only), left / right = the argmax rows
 *       of classes left / right (first maximum, NaN highest).  Writes indices [N, 3] int64 (left, right, object; may be
 *       NULL) and reference_points [N, 3, 2] = means of sigmoid over the x / y columns of the gathered rows (left, right
 *       from hand, object from obj).  Every class index must be < K; at most 14 object classes.  One launch per call. */
int msda_assembly_refine_f32(const float *reference_points, int width, const float *cls, int K, const float *keypoints, long long M,
                             float *out, msda_stream_t stream);
int msda_assembly_proposals_f32(const float *memory, long long memory_frame_stride, const uint8_t *padding_mask,
                                long long mask_frame_stride, int N, int H, int W, int C, float *proposals, float *memory_out,
                                uint8_t *row_mask, msda_stream_t stream);
int msda_assembly_select_f32(const float *cls, const float *hand, const float *obj, int N, int S, int K, int obj_first, int obj_last,
                             int left, int right, int64_t *indices, float *reference_points, msda_stream_t stream);

/* ---- The DINO decoder's query positions and refinement (models/dino/deformable_transformer.py:730-746, :781-798) ----------
 * Added after MSDA_ABI_VERSION 116 without a version bump: the five entries below are purely additive (no existing
 * declaration changed), so a binding compiled against 116 keeps working; callers probe them by symbol.
 *
 * Rows are sequence-first: ref [M, width] (width 2 or 42, 1 or 21 (x, y) pairs) with row m in frame m % N, so M % N == 0;
 * valid_xy [N, 2] the level-0 valid ratios (x, y), NULL = 1; dim_t [64] torch's table at even indices (utils.py:142-143).
 * All fp32, contiguous rows.
 *   msda_dino_sine_embed_f32   gen_sineembed_for_position (utils.py:138-165) of ref * valid ratios: pe [M, 256] (16-byte
 *       aligned); ex = 2 pi * mean_k(ref[m, 2k] * valid_x), ey likewise from the odd columns; pe[m, 2i + s] = s ?
 *       cos(ey / dim_t[i]) : sin(ey / dim_t[i]) for i < 64, columns 128 .. 255 the same from ex (y first).  One launch.
 *   msda_dino_query_pos_forward_f32  ref_point_head of that table in one launch: h [M, 256] = relu(pe @ w1^T + b1), y [M, 256]
 *       = h @ w2^T + b2, with w1, w2 [256, 256] (16-byte aligned) and b1, b2 [256].  The table never exists in memory and h is
 *       written exactly once.  fp32 MFMA, fixed summation order.  msda_dino_query_pos_supported(width, N, M, hidden, out)
 *       tells beforehand (1 = the call runs): hidden = out = 256 only.
 *   msda_dino_refine_forward_f32   the refinement (:781-798) without its boolean-mask adds: ref, delta_key, delta_obj [M, 42],
 *       cls [M, K]; per row c = argmax(cls) (first maximum, NaN highest), code = 2 if c is hand0 / hand1, 1 if c is neither and
 *       not 0, else 0; u = inverse_sigmoid(ref) (util/misc.py:614-618) + (code 1: delta_obj, code 2: delta_key);
 *       out [M, 42] = sigmoid(u) * 2 - 1, code [M] bytes.  One launch, no synchronisation.
 *   msda_dino_refine_backward_f32  g_u = grad_out * (1 - out^2) / 2; grad_key = g_u where code == 2, else 0; grad_obj = g_u
 *       where code == 1, else 0 (either may be NULL: not written).  cls and ref get no gradient.  One launch.
 * No allocation, no synchronisation, no atomics: bitwise reproducible, capturable in a graph.  Argument errors
 * (MSDA_ERR_ARGUMENT before any launch): width not 2 or 42, N <= 0, M % N != 0, K < 1, tensors beyond 2^31 elements, a null
 * or misaligned pointer. */
int msda_dino_sine_embed_f32(const float *ref, int width, const float *valid_xy, int N, long long M, const float *dim_t, float *pe,
                             msda_stream_t stream);
int msda_dino_query_pos_supported(int width, int N, long long M, int hidden, int out_features);
int msda_dino_query_pos_forward_f32(const float *ref, int width, const float *valid_xy, int N, long long M, const float *dim_t,
                                    const float *w1, const float *b1, const float *w2, const float *b2, float *h, float *y,
                                    msda_stream_t stream);
int msda_dino_refine_forward_f32(const float *ref, const float *cls, int K, const float *delta_key, const float *delta_obj, int hand0,
                                 int hand1, long long M, float *out, uint8_t *code, msda_stream_t stream);
int msda_dino_refine_backward_f32(const float *grad_out, const float *out, const uint8_t *code, long long M, float *grad_key,
                                  float *grad_obj, msda_stream_t stream);

/* ---- DINO's two-stage query selection (models/dino/deformable_transformer.py:348-387) -------------------------------------
 * Added after MSDA_ABI_VERSION 116 without a version bump: the four entries below are purely additive (no existing
 * declaration changed), so a binding compiled against 116 keeps working; callers probe them by symbol.
 *
 * The rule is msda_two_stage_select_f32's, for any number of rows per frame: per frame the Q rows with the largest max_k
 * cls[n, s, k], descending; ties: the lower row first; NaN above every number, -0 equal to +0; per-row max / argmax as
 * torch.max(-1) / argmax(-1) (first maximum; NaN wins).
 *   msda_dino_select_supported(S, K, Q, C)  1 = the kernels take it: 1 <= Q <= min(S, 2048), S <= 1048576, 1 <= K <= 256,
 *       C a multiple of 4 in 4..2048.
 *   msda_dino_select_workspace_bytes(N, S)  the size of `workspace` (a host function of N and S; 0 for an empty problem).
 *   msda_dino_select_forward_f32   cls [N, S, K], memory [N, S, C], proposals [N, S, 42], all fp32 contiguous.  Replaces the
 *       torch.topk of :349, the class gather of :353-355, the gathers of :369 and :387 and — with the caller's two
 *       torch.where — the boolean-mask assignments of :376-377 (a nonzero and a host synchronisation each).  Writes topk
 *       [N, Q] int64; slot [N, S] int32, the inverse map (q at a selected row, -1 elsewhere: every element written); tgt
 *       [N, Q, C], the selected rows of memory (:387); prop_sel [N, Q, 42], the selected rows of proposals (:369; +inf rows are
 *       copied as +inf); code [N, Q] bytes: 2 if the row's class argmax is hand_class0 / hand_class1, 1 if it is neither and
 *       not 0, else 0 (:353-355).  Two launches: the rows' keys, then one workgroup per frame (radix select of the Q-th key,
 *       a sort of the Q selected keys, the gathers).  memory, tgt and workspace 16-byte aligned.
 *   msda_dino_select_backward_f32  the gradient of tgt with respect to memory (the gather of :387): grad_memory [N, S, C] =
 *       grad_tgt[n, slot[n, s]] where slot >= 0, else 0.  Every element is written by the one launch: no memset before it.
 *       grad_tgt and grad_memory 16-byte aligned.
 * No allocation, no synchronisation, integer LDS atomics only: bitwise reproducible, capturable in a graph.  Argument
 * errors (MSDA_ERR_ARGUMENT before any launch): Q > S, sizes msda_dino_select_supported refuses, N above 65535, tensors
 * beyond 2^31 elements, a null or misaligned pointer with N > 0.  N == 0 returns MSDA_OK. */
int msda_dino_select_supported(int S, int K, int Q, int C);
unsigned long long msda_dino_select_workspace_bytes(int N, int S);
int msda_dino_select_forward_f32(const float *cls, const float *memory, const float *proposals, int N, int S, int K, int Q, int C,
                                 int hand_class0, int hand_class1, int64_t *topk, int32_t *slot, float *tgt, float *prop_sel,
                                 uint8_t *code, void *workspace, msda_stream_t stream);
int msda_dino_select_backward_f32(const int32_t *slot, const float *grad_tgt, int N, int S, int Q, int C, float *grad_memory,
                                  msda_stream_t stream);

/* ---- DINO's contrastive-denoising queries (models/dino/dn_components.py:20-150, prepare_for_cdn) ---------------------------
 * Added after MSDA_ABI_VERSION 116 without a version bump: the three entries below are purely additive (no existing
 * declaration changed), so a binding compiled against 116 keeps working; callers probe them by symbol.
 *
 * The targets are the matcher's packed form: labels [T] int64, offsets [B + 1] int64 (frame b owns targets offsets[b] ..
 * offsets[b + 1] - 1), keypoints [T, width] fp32; weight [rows_book, hidden] fp32 is label_enc's table (16-byte aligned).
 * single_pad (the largest target count of a frame), groups (dn_number after the division of :46-58) and so every shape are
 * HOST values (:49-58 read them back from the device); pad = 2 * single_pad * groups.
 *   msda_cdn_supported(hidden, width, rows_book, E)   1 = the kernels take it: hidden a multiple of 4 in 4..1024, width in
 *       1..64, rows_book >= 1, rows_book * hidden < 2^31, and every draw counter of E = 2 * groups * T flat elements below
 *       2^32: 2 E (1 + width) < 2^32.
 *   msda_cdn_prepare_forward_f32   ONE launch writes every element of input_query_label [B, pad, hidden], input_query_key
 *       [B, pad, width] and noised_labels [B, pad] int32 (:107-123; no memset).  Row (b, r * single_pad + j) with
 *       j < offsets[b + 1] - offsets[b] holds target t = offsets[b] + j in repetition r of 2 * groups (:67-70, :119-120; even r
 *       = positive_idx, odd r = negative_idx, :82-85): weight[label'] (:108), inverse_sigmoid(key') (:109, util/misc.py:614-618)
 *       and label'; the other rows are zero with label -1 (:111-115), as is a row whose offsets or label do not address the
 *       tables.  Draws (:74-78, :94-103), from the library's counter hash with base = mix(seed[0], 0), flat element
 *       e = r * T + t: label' = (hash(base + 2e + 1) * num_classes) >> 32 iff hash(base + 2e) < flip_threshold, else the
 *       label (flip_threshold 0: no draw).  key_noise_scale > 0 (the noise the reference computes at :94-103 and drops,
 *       :104-105): for column c with k = 2E + 2 (e * width + c): sign = hash(base + k) >> 31 ? +1 : -1, u = (hash(base + k +
 *       1) >> 8) * 2^-24, part = (u + (r odd ? 1 : 0)) * sign, key' = clamp(key + (part * key) * key_noise_scale, 0, 1), each
 *       product and sum rounded on its own; key_noise_scale 0: key' = key.  seed: device int64, NULL allowed when nothing is
 *       drawn.  key_debug (tests; NULL = not written): key' [B, pad, width] before inverse_sigmoid, 0 in padding rows.
 *   msda_cdn_prepare_backward_f32  ONE launch: grad_weight [rows_book, hidden] (16-byte aligned, every element written)
 *       = per class c the sum of the rows of grad_label [rows, hidden] whose noised_labels [rows] equal c, summed in an order
 *       that depends on the labels alone (:108's embedding backward without atomics): bitwise reproducible.
 * No allocation, no synchronisation, no atomics, capturable in a graph.  Argument errors (MSDA_ERR_ARGUMENT before any launch):
 * sizes outside msda_cdn_supported, negative sizes, groups or num_classes < 1, num_classes > rows_book, key_noise_scale < 0,
 * tensors beyond 2^31 elements, draws without a seed, a null or misaligned pointer.  pad == 0: MSDA_OK, no launch. */
int msda_cdn_supported(int hidden, int width, long long rows_book, long long E);
int msda_cdn_prepare_forward_f32(const int64_t *labels, const int64_t *offsets, const float *keypoints, const float *weight,
                                 const long long *seed, int B, long long T, int width, int hidden, long long rows_book,
                                 int single_pad, int groups, int num_classes, unsigned flip_threshold, float key_noise_scale,
                                 float *input_query_label, float *input_query_key, int32_t *noised_labels, float *key_debug,
                                 msda_stream_t stream);
int msda_cdn_prepare_backward_f32(const float *grad_label, const int32_t *noised_labels, long long rows, int hidden,
                                  long long rows_book, float *grad_weight, msda_stream_t stream);

/* ---- The Hungarian matchers (models/matcher.py: ArcticMatcher :20-125, AssemblyMatcher :128-230) -------------------------
 * Added after MSDA_ABI_VERSION 116 without a version bump: the three entries below are purely additive (no existing
 * declaration changed), so a binding compiled against 116 keeps working; callers probe them by symbol.
 *
 *   msda_match_arctic_f32    one launch matches `sets` prediction sets (HOST arrays of `sets` device pointers, sets <= 16):
 *       pred_logits [bs, Q, K], pred_hand_key / pred_obj_key [bs, Q, D] (Q <= 1024, D <= 64; ignored, D = 0, when
 *       keypoints is NULL), all fp32 contiguous, against the targets of every frame: labels [n_targets] int64, keypoints
 *       [n_targets, D] fp32 or NULL, offsets [bs + 1] int64 (frame f owns targets offsets[f]..offsets[f+1]-1, at most
 *       t_max <= 16 of them) and is_valid [bs] int32 (non-zero = valid).  Output slot k of every set pairs output frame k
 *       with the k-th VALID frame's targets, as the reference's split does (:122-123).  Per slot, on chip: the cost block
 *       C = cost_keypoint * L1 + cost_class * (focal pos - neg) (L1 against the hand head for labels 12 / 13, none for
 *       label 0, the object head otherwise; no L1 term without keypoints) and scipy's linear_sum_assignment of it (the
 *       same shortest augmenting path with fp64 duals and scipy's tie rule).
 *       out int64 [2 * sets * bs * t_max + 2 * sets * bs + 1]: query_idx [sets, bs, t_max] (ascending), target_idx
 *       [sets, bs, t_max] (-1 padding), count [sets, bs] (min(Q, T); -1 past the valid frames), status [sets, bs]
 *       (0 ok, 1 a NaN or -inf cost, 2 infeasible, 3 a label outside [0, K), 4 offsets outside [0, n_targets] or a frame
 *       above t_max targets), and the number of valid frames.  cost_debug [sets, bs, Q, t_max] fp32 or NULL receives
 *       each block (entries past a frame's targets are not written).  One launch, no synchronisation, nothing read on
 *       the host; bs = 0 launches nothing.
 *   msda_match_assembly_f32  the same for AssemblyMatcher: one keypoint head pred_keypoints [bs, Q, D], L1 where the label
 *       is not 0, no is_valid (slot k = frame k; the last output word is bs).
 *   msda_lsap_f32            scipy's linear_sum_assignment of B fp32 blocks cost [B, Q, T] (min(Q, T) <= 16,
 *       max(Q, T) <= 1024) with the same solver; out int64 [2 * B * W + 2 * B], W = min(Q, T): row (query) indices
 *       ascending, column indices, count and status per block as above. */
int msda_match_arctic_f32(const float *const *pred_logits, const float *const *pred_hand_key, const float *const *pred_obj_key,
                          int sets, int bs, int Q, int K, int D, const int64_t *labels, const float *keypoints,
                          const int64_t *offsets, long long n_targets, const int32_t *is_valid, int t_max, float cost_class,
                          float cost_keypoint, int64_t *out, float *cost_debug, msda_stream_t stream);
int msda_match_assembly_f32(const float *const *pred_logits, const float *const *pred_keypoints, int sets, int bs, int Q, int K,
                            int D, const int64_t *labels, const float *keypoints, const int64_t *offsets, long long n_targets,
                            int t_max, float cost_class, float cost_keypoint, int64_t *out, float *cost_debug,
                            msda_stream_t stream);
int msda_lsap_f32(const float *cost, int B, int Q, int T, int64_t *out, msda_stream_t stream);

/* ---- The set criteria's matched losses (models/actic_detr.py SetArcticCriterion :365-569, models/assembly_detr.py
 * SetAssemblyCriterion :248-446) over the matcher's device result ------------------------------------------------------------
 * Added after MSDA_ABI_VERSION 116 without a version bump, as the matcher block above: purely additive entries.
 *
 *   msda_criterion_fwd_f32  one launch, one workgroup per prediction set.  kind 0 = ARCTIC, 1 = AssemblyHands.  HOST arrays
 *       of `sets` device pointers (sets <= 16): pred_logits [bs, Q, K] and, with target keypoints, pred_hand_key [bs, Q, D]
 *       (AssemblyHands: pred_keypoints) and pred_obj_key [bs, Q, D] (ARCTIC only; NULL for AssemblyHands), all fp32
 *       contiguous.  match: the int64 result of msda_match_{arctic,assembly}_f32 for the same sets and t_max.  The targets as
 *       for the matcher (labels, keypoints [n_targets, D] or NULL with D = 0, offsets [bs + 1], is_valid [bs] for ARCTIC:
 *       slot k pairs with the k-th valid frame; NULL for AssemblyHands), joint_valid uint8 [n_targets, D] (AssemblyHands
 *       with keypoints, else NULL), hand_mask (bit l for each hand label l < 64: 12 and 13 for ARCTIC, cfg.hand_idx for
 *       AssemblyHands), num_boxes a device fp32 scalar, focal_alpha.
 *       losses fp32 [sets, 4]: ARCTIC loss_ce, loss_hand_keypoint, loss_obj_keypoint, cardinality_error (all 0 when no
 *       valid frame has a target); AssemblyHands loss_ce, loss_hand_keypoint, cardinality_error, class_error.
 *       stats int32 [sets, 4]: status bits (1 a matched label outside [0, K), 2 offsets / target indices that do not
 *       describe the targets, 4 AssemblyHands joint_valid mask mismatch: a matched label outside hand_mask or a frame
 *       with unmatched targets, loss_hand_keypoint is then nan, 8 a matcher slot status), hand rows, object rows, and 1
 *       when no valid frame has a target (ARCTIC).  Reductions in a fixed order: bitwise reproducible.
 *   msda_criterion_bwd_f32  one launch: from grad_losses fp32 [sets, 4] (the forward's columns; cardinality_error and
 *       class_error get none) and the forward's stats, writes every element of grad_logits and, with keypoints, of
 *       grad_hand_key / grad_obj_key (HOST arrays of device pointers shaped as the predictions): zero except matched rows.
 *   Limits: 1 <= bs <= 1024, 1 <= Q, 1 <= K, 0 <= t_max <= 16.  No synchronisation, nothing read on the host. */
#define MSDA_CRITERION_ARCTIC 0
#define MSDA_CRITERION_ASSEMBLY 1
int msda_criterion_fwd_f32(int kind, const float *const *pred_logits, const float *const *pred_hand_key,
                           const float *const *pred_obj_key, int sets, int bs, int Q, int K, int D, const int64_t *match,
                           int t_max, const int64_t *labels, const float *keypoints, const int64_t *offsets,
                           long long n_targets, const int32_t *is_valid, const uint8_t *joint_valid,
                           unsigned long long hand_mask, const float *num_boxes, float focal_alpha, float *losses,
                           int32_t *stats, msda_stream_t stream);
int msda_criterion_bwd_f32(int kind, const float *const *pred_logits, const float *const *pred_hand_key,
                           const float *const *pred_obj_key, int sets, int bs, int Q, int K, int D, const int64_t *match,
                           int t_max, const int64_t *labels, const float *keypoints, const int64_t *offsets,
                           long long n_targets, const int32_t *is_valid, const uint8_t *joint_valid,
                           unsigned long long hand_mask, const float *num_boxes, float focal_alpha,
                           const float *grad_losses, const int32_t *stats, float *const *grad_logits,
                           float *const *grad_hand_key, float *const *grad_obj_key, msda_stream_t stream);

/* ---- The DINO criterion's matched and denoising losses (models/dino/dino.py SetCriterion: loss_labels, loss_cardinality and
 * loss_boxes :453-532, the denoising losses :615-664) --------------------------------------------------------------------------
 * Added after MSDA_ABI_VERSION 116 without a version bump, as the matcher and criterion blocks above: purely additive entries;
 * msda_criterion_fwd_f32 / msda_criterion_bwd_f32 are unchanged.
 *
 *   msda_criterion_dino_fwd_f32  `sets` <= 16 prediction sets that may differ in query count.  HOST arrays of length `sets`,
 *       read at call time into the kernels' argument record: device pointers pred_logits [bs, Q[s], K] and, with target
 *       keypoints, pred_hand_key / pred_obj_key [bs, Q[s], D] (fp32 contiguous; NULL arrays with D = 0 otherwise), the query
 *       counts Q[s], and match_set[s]: the set's index inside `match` (the int64 result of msda_match_arctic_f32 for
 *       match_sets sets and t_max), or -1 for a DENOISING set, which needs Q[s] = groups * single_pad and reads no match
 *       buffer (match may be NULL when every set is one).  The targets as for the matcher (labels, keypoints [n_targets, D]
 *       or NULL, offsets [bs + 1], is_valid [bs]), hand_mask (bit l for each hand label l < 64), num_boxes a device fp32
 *       scalar, focal_alpha.  Slot k of every set pairs output frame k with the k-th valid frame f's n_f targets: a matched
 *       set through slot k of its matcher set; a denoising set pairs query g * single_pad + j with target offsets[f] + j for
 *       every g < groups and j < n_f (:623-633).  n_f > single_pad / 2 sets status bit 2 and the frame gives no pair.
 *       losses fp32 [sets, 4]: loss_ce = focal(alpha, gamma 2).mean(1).sum() / num_boxes * Q[s] (a denoising set divides by
 *       num_boxes * groups), loss_hand_keypoint (L1 of the hand head over paired rows with a hand label / their count / 21;
 *       0 without one), loss_obj_keypoint (the object head over the other paired rows / their count / 21; 0 / 0 = nan
 *       without one), cardinality_error (mean over frames f of |#(argmax of output frame f's rows != K - 1) - n_f|: the
 *       empty class is K - 1).  Every term is 0 when no valid frame has a target.  stats int32 [sets, 4]: status bits (1 a
 *       paired label outside [0, K), 2 offsets / target indices that do not describe the targets, 8 a matcher slot status),
 *       hand rows, object rows, and 1 when no valid frame has a target.
 *       Two launches: one workgroup per chunk (up to MSDA_CRITERION_DINO_CHUNK_ROWS rows of one set and output frame)
 *       writes a record of fp64 partial sums and integer counts to `workspace` (8-byte aligned, at least
 *       MSDA_CRITERION_DINO_PARTIAL_BYTES * bs * sum over s of ceil(Q[s] / MSDA_CRITERION_DINO_CHUNK_ROWS) bytes), then one
 *       workgroup per set adds its records in a fixed order.  No float atomics: bitwise reproducible, and a set's row does
 *       not depend on the other sets of the call.
 *   msda_criterion_dino_bwd_f32  one launch: from grad_losses fp32 [sets, 4] (cardinality_error gets none) and the forward's
 *       stats, writes every element of grad_logits and, with keypoints, of grad_hand_key / grad_obj_key (HOST arrays of
 *       device pointers shaped as the predictions): zero except paired rows.
 *   Limits: 1 <= bs <= 1024, 1 <= Q[s], 1 <= K, 0 <= t_max <= 16, bs * Q[s] * max(K, D) < 2^31.  No allocation, no
 *   synchronisation, nothing read on the host; argument errors return MSDA_ERR_ARGUMENT before any launch. */
#define MSDA_CRITERION_DINO_CHUNK_ROWS 256
#define MSDA_CRITERION_DINO_PARTIAL_BYTES 64
int msda_criterion_dino_fwd_f32(const float *const *pred_logits, const float *const *pred_hand_key,
                                const float *const *pred_obj_key, const int *Q, const int *match_set, int sets, int bs, int K,
                                int D, int single_pad, int groups, const int64_t *match, int match_sets, int t_max,
                                const int64_t *labels, const float *keypoints, const int64_t *offsets, long long n_targets,
                                const int32_t *is_valid, unsigned long long hand_mask, const float *num_boxes,
                                float focal_alpha, void *workspace, unsigned long long workspace_bytes, float *losses,
                                int32_t *stats, msda_stream_t stream);
int msda_criterion_dino_bwd_f32(const float *const *pred_logits, const float *const *pred_hand_key,
                                const float *const *pred_obj_key, const int *Q, const int *match_set, int sets, int bs, int K,
                                int D, int single_pad, int groups, const int64_t *match, int match_sets, int t_max,
                                const int64_t *labels, const float *keypoints, const int64_t *offsets, long long n_targets,
                                const int32_t *is_valid, unsigned long long hand_mask, const float *num_boxes,
                                float focal_alpha, const float *grad_losses, const int32_t *stats, float *const *grad_logits,
                                float *const *grad_hand_key, float *const *grad_obj_key, msda_stream_t stream);

/* ---- The DeformableDETR prediction heads (models/actic_detr.py DeformableDETR.forward :245-287, models/assembly_detr.py
 * DeformableDETR.forward :172-210) as grouped fp32 GEMMs --------------------------------------------------------------------
 * Added after MSDA_ABI_VERSION 116 without a version bump: purely additive entries.
 *
 * Per decoder level l < L (M = B * Q rows, hidden C): the class Linear (K classes), n_mlp 3-layer keypoint MLPs C -> C -> C ->
 * D (ARCTIC: key_embed, obj_key_embed, D = 42, n_mlp 2 for two-stage models, 0 otherwise; AssemblyHands: keypoint_embed,
 * D = 63, n_mlp 1) and, ARCTIC only, the six shared Linears mano_pose 48, mano_beta 10, hand_cam 3, obj_cam 3, obj_rot 3,
 * obj_rad 1 (:264-270).  Keypoint epilogues: ARCTIC sigmoid(y + inverse_sigmoid(ref)) * 2 - 1 (:250-256); AssemblyHands adds
 * inverse_sigmoid(ref) (2-d) or the means of its 21 x / 21 y values (42-d) to the x and y of each of the 21 points, then
 * sigmoid * 2 - 0.5 (:186-206).  ref is init_ref [M, R] for level 0 and inter_ref [L - 1, M, R] after (AssemblyHands
 * maps those r -> (r + 0.5) / 2 first, :180).  All tensors fp32 contiguous, hs [L, M, C]; C % 4 == 0, 4 <= C <= 4096,
 * 1 <= L <= 8, L * M * max(C, K) < 2^31.
 *   HOST pointer arrays: cls_w / cls_b [L] ([1] with MSDA_HEADS_SHARED_CLS: one module repeated over the levels),
 *   mlp_w / mlp_b [n_mlp * 3 * L] at (head * 3 + layer) * L + l ([n_mlp * 3], index head * 3 + layer, with
 *   MSDA_HEADS_SHARED_MLP), shared_w / shared_b [6] (ARCTIC; NULL for AssemblyHands).  Weights [n_out, n_in] as nn.Linear.
 *
 *   msda_heads_forward_f32   at most 3 launches (one per MLP depth, every head of every level in each).  Writes logits
 *       [L, M, K], kp_out[h] [L, M, D], shared_out[g] [L, M, n_g] (the reference's torch.stack'ed tensors), and saves the
 *       hidden activations hidden [n_mlp, 2, L, M, C] and the keypoint sigmoids sig [n_mlp, L, M, D] for the backward.
 *   msda_heads_backward_f32  at most 5 launches: input gradients per depth (the depth-1 one reduces over every head that
 *       reads hs[l]; ReLU masks from the saved activations), one grouped weight-gradient pass in row chunks, one chunk-ordered
 *       reduce.  Writes every element of grad_hs [L, M, C] and of every weight / bias gradient (host arrays shaped as the
 *       weights').  workspace: at least msda_heads_workspace_bytes(...) bytes.
 *   msda_heads_supported     1 when the kernels take hidden size C.
 * Fixed summation order: bitwise reproducible.  No allocation, no synchronisation; argument errors before any launch. */
#define MSDA_HEADS_ARCTIC 0
#define MSDA_HEADS_ASSEMBLY 1
#define MSDA_HEADS_SHARED_CLS 1u
#define MSDA_HEADS_SHARED_MLP 2u
int msda_heads_supported(int C);
unsigned long long msda_heads_workspace_bytes(int kind, int L, long long M, int C, int K, int n_mlp, unsigned flags);
int msda_heads_forward_f32(int kind, int L, long long M, int C, int K, int n_mlp, int R, unsigned flags, const float *hs,
                           const float *init_ref, const float *inter_ref, const float *const *cls_w,
                           const float *const *cls_b, const float *const *mlp_w, const float *const *mlp_b,
                           const float *const *shared_w, const float *const *shared_b, float *logits, float *const *kp_out,
                           float *const *shared_out, float *hidden, float *sig, msda_stream_t stream);
int msda_heads_backward_f32(int kind, int L, long long M, int C, int K, int n_mlp, int R, unsigned flags, const float *hs,
                            const float *init_ref, const float *inter_ref, const float *const *cls_w,
                            const float *const *cls_b, const float *const *mlp_w, const float *const *mlp_b,
                            const float *const *shared_w, const float *const *shared_b, const float *hidden,
                            const float *sig, const float *grad_logits, const float *const *grad_kp,
                            const float *const *grad_shared, float *grad_hs, float *const *grad_cls_w,
                            float *const *grad_cls_b, float *const *grad_mlp_w, float *const *grad_mlp_b,
                            float *const *grad_shared_w, float *const *grad_shared_b, void *workspace,
                            unsigned long long workspace_bytes, msda_stream_t stream);

/* The reference gradient of the ARCTIC keypoint epilogue, for callers whose references carry a gradient: DINO's decoder hands
 * its refined reference points on undetached, and models/dino/dino.py:333-334 feed them to
 * (delta + inverse_sigmoid(ref)).sigmoid() * 2 - 1 (util/misc.py inverse_sigmoid).  Added after MSDA_ABI_VERSION 116 without a
 * version bump: a purely additive entry beside msda_heads_backward_f32, which stops at delta.
 * For every level whose reference needs a gradient and every element e = (level row, j), j < R = 42:
 *   grad_ref[e] = dinv(ref[e]) * sum over the n_mlp = 2 heads h of (grad_kp[h][e] * 2) * (1 - sig[h][e]) * sig[h][e]
 *   dinv(x)     = [0 <= x <= 1] * ([x >= eps] / max(x, eps) + [1 - x >= eps] / max(1 - x, eps)),  eps = 1e-5f
 * (what autograd makes of inverse_sigmoid's three clamps and its log: torch's clamp passes the gradient at its bounds; the head
 * terms in the order and grouping of the backward's depth-3 operand).  init_ref [M, R], inter_ref [L - 1, M, R], the forward's
 * saved sig [n_mlp, L, M, R], grad_kp: HOST array of the n_mlp gradients [L, M, R]; all fp32 contiguous.  grad_init_ref [M, R]
 * and grad_inter_ref [L - 1, M, R] may each be NULL: that reference needs no gradient, and nothing of its levels is read (its
 * reference pointer may be NULL too).  Every element of a non-NULL output is written.  1 <= L <= 8, M >= 1, R == 42,
 * n_mlp == 2, L * M * R < 2^31.  One launch (none when both outputs are NULL); no atomics, fixed order: bitwise
 * reproducible.  No allocation, no synchronisation; argument errors before any launch. */
int msda_heads_ref_backward_f32(int L, long long M, int n_mlp, int R, const float *init_ref, const float *inter_ref,
                                const float *sig, const float *const *grad_kp, float *grad_init_ref, float *grad_inter_ref,
                                msda_stream_t stream);

/* The bf16-autocast form of the same node.  Added after MSDA_ABI_VERSION 116 without a version bump: purely additive entries.
 * Same problems, host pointer arrays, launch budget (3 forward, 5 backward) and flags as the fp32 entries; every product runs
 * on the bf16 MFMA with fp32 accumulation, and the dtypes and roundings are those of torch's bf16 autocast over the
 * reference's composition.  bf16 tensors are uint16_t bit patterns; a `void *` is float for MSDA_HEADS_ARCTIC and bf16 for
 * MSDA_HEADS_ASSEMBLY.
 *   fp32: hs, every weight and bias, init_ref, inter_ref, sig, grad_hs and every weight / bias gradient.  hs and the weights
 *         are rounded to bf16 (nearest even) in the load that stages them; nothing else reads them.
 *   bf16: hidden [n_mlp, 2, L, M, C], shared_out[g] and grad_shared[g], the hidden gradients in the workspace.
 *   kind: logits / grad_logits, kp_out[h] / grad_kp[h].  ARCTIC: logits are bf16-rounded values stored as float (the
 *         reference's .to(float32)); keypoints are sigmoid(float(rnd(y)) + inverse_sigmoid(ref)) * 2 - 1 in fp32.
 *         AssemblyHands: rnd(rnd(rnd(s) * 2) - 0.5), s = sigmoid of the bf16 pre-activation after rnd(y + offset) on x and y.
 *   Every Linear output is rounded once to bf16, bias included; ReLU acts on bf16.  Backward: dy o mode is formed in fp32 and
 *   rounded to bf16 as a matrix operand; hidden gradients are stored bf16; grad_hs and the weight / bias gradients are
 *   accumulated and written in fp32 without a bf16 rounding.
 * C % 8 == 0, 8 <= C <= 4096 (msda_heads_bf16_supported); hs, hidden, the weights and the workspace 16-byte aligned; the other
 * limits of the fp32 entries.  workspace: at least msda_heads_bf16_workspace_bytes(...) bytes.
 * Fixed summation order: bitwise reproducible.  No allocation, no synchronisation; argument errors before any launch. */
int msda_heads_bf16_supported(int C);
unsigned long long msda_heads_bf16_workspace_bytes(int kind, int L, long long M, int C, int K, int n_mlp, unsigned flags);
int msda_heads_forward_bf16(int kind, int L, long long M, int C, int K, int n_mlp, int R, unsigned flags, const float *hs,
                            const float *init_ref, const float *inter_ref, const float *const *cls_w,
                            const float *const *cls_b, const float *const *mlp_w, const float *const *mlp_b,
                            const float *const *shared_w, const float *const *shared_b, void *logits, void *const *kp_out,
                            uint16_t *const *shared_out, uint16_t *hidden, float *sig, msda_stream_t stream);
int msda_heads_backward_bf16(int kind, int L, long long M, int C, int K, int n_mlp, int R, unsigned flags, const float *hs,
                             const float *init_ref, const float *inter_ref, const float *const *cls_w,
                             const float *const *cls_b, const float *const *mlp_w, const float *const *mlp_b,
                             const float *const *shared_w, const float *const *shared_b, const uint16_t *hidden,
                             const float *sig, const void *grad_logits, const void *const *grad_kp,
                             const uint16_t *const *grad_shared, float *grad_hs, float *const *grad_cls_w,
                             float *const *grad_cls_b, float *const *grad_mlp_w, float *const *grad_mlp_b,
                             float *const *grad_shared_w, float *const *grad_shared_b, void *workspace,
                             unsigned long long workspace_bytes, msda_stream_t stream);

/* ---- The layers' FFN under bf16 autocast: linear2(dropout(relu(linear1(x)))) of every encoder and decoder layer
 * (models/arctic_transformer.py:283-287, :366-370) -------------------------------------------------------------------------
 * Added after MSDA_ABI_VERSION 116 without a version bump: purely additive entries.
 *
 * x [M, C] (fp32, or bf16 bits when x_is_bf16), w1 [F, C], b1 [F], w2 [C, F], b2 [C] fp32; a [M, F] and y [M, C] bf16 bits.
 * Every product runs on the bf16 MFMA with fp32 accumulation; x, w1 and w2 are rounded to bf16 (nearest even) in the loads that
 * stage them.  h = rnd(x . w1^T + b1) (fp32 bias, one rounding; never stored), a = rnd(relu(h) * keep / (1 - p)),
 * y = rnd(a . w2^T + b2).  p == 0: no dropout (evaluation); p > 0: keep is a hash of (*seed, row * F + column) (seed: device),
 * not nn.Dropout's stream, and the backward reads a > 0 instead of a mask.
 *   msda_ffn_forward_bf16   (models/arctic_transformer.py:283-287, :366-370) ONE launch.  Writes a, y and, for an fp32 x, its
 *       bf16 rounding xb [M, C] (null for a bf16 x, which is then the backward's xb itself).
 *   msda_ffn_backward_bf16  (the gradient of models/arctic_transformer.py:283-287, :366-370) at most 5 launches:
 *       gh = rnd((grad_out . w2) / (1 - p) * [a > 0]) (bf16, in the workspace), grad_x = gh . w1 (fp32, or rounded once to bf16
 *       when grad_x_is_bf16), the two weight gradients' first stages (grad_w2 = grad_out^T . a, grad_w1 = gh^T . xb, fp32 with
 *       their bias gradients, as msda_linear_wgrad_multi) and their one second stage.  A null grad_x, grad_w1 (with grad_b1) or
 *       grad_w2 (with grad_b2) is not computed; gh only when grad_x or grad_w1 is asked for.  workspace: at least
 *       msda_ffn_bf16_workspace_bytes(M, C, F) bytes (gh and the weight gradients' partial sums).
 *   msda_ffn_bf16_supported (models/arctic_transformer.py:283-287, :366-370: C = 256, F = 1024 or 2048) 1 when C % 64 == 0,
 *       64 <= C <= 256, F % 64 == 0 and 64 <= F <= 8192.
 *   msda_ffn_bf16_workspace_bytes  (the backward of models/arctic_transformer.py:283-287, :366-370) 0 for sizes the entries
 *       refuse.
 * M >= 1, M * F < 2^31, 0 <= p < 1; x, xb, a, y, grad_out, grad_x, the weights and the workspace 16-byte aligned.
 * Fixed summation order: bitwise reproducible.  No allocation, no synchronisation; argument errors before any launch. */
int msda_ffn_bf16_supported(int C, int F);
unsigned long long msda_ffn_bf16_workspace_bytes(long long M, int C, int F);
int msda_ffn_forward_bf16(long long M, int C, int F, const void *x, int x_is_bf16, const float *w1, const float *b1, const float *w2,
                          const float *b2, double p, const long long *seed, uint16_t *xb, uint16_t *a, uint16_t *y,
                          msda_stream_t stream);
int msda_ffn_backward_bf16(long long M, int C, int F, const uint16_t *grad_out, const uint16_t *xb, const uint16_t *a, const float *w1,
                           const float *w2, double p, void *grad_x, int grad_x_is_bf16, float *grad_w1, float *grad_b1,
                           float *grad_w2, float *grad_b2, void *workspace, unsigned long long workspace_bytes, msda_stream_t stream);

/* ---- SmoothNet (models/smoothnet.py:7-178): MotionSmoother modules as grouped fp32 GEMMs, and get_arctic_item's query
 * selection (arctic_tools/process.py:20-70) ---------------------------------------------------------------------------------
 * Added after MSDA_ABI_VERSION 116 without a version bump: purely additive entries.
 *
 * Smoother geometry: window T, output size O, hidden H, residual hidden R, num_blocks nb (3 <= T, O <= 4096, H and R multiples
 * of 4 in [4, 4096], nb <= 4); n_mod <= 6 MotionSmoother modules; n_calls <= 12 calls, call i runs module call_mod[i] (at
 * most 4 calls per module) on x[i] [call_B[i] * T, call_C[i]] (the reference's view(B, T, C)) and writes out[i]
 * [call_B[i] * O, call_C[i]].  params: HOST array of n_mod * (3 * (4 + 4 * nb) + 2) pointers, each module's parameters in its
 * parameters() order (pos, vel, acc Smoothers: encoder weight, bias, per block linear1 weight, bias, linear2 weight, bias,
 * decoder weight, bias; then fusion weight, bias), hidden-layer weights 16-byte aligned.  Dropout (training != 0 and p > 0):
 * keep probability 1 - p, scale 1 / (1 - p), the mask a hash of (*seed, problem = module * 3 + smoother, layer, module row,
 * column) — layer 2j - 1 / 2j: the two Linears of block j — regenerated in the backward; not nn.Dropout's stream.
 *   msda_smoother_workspace_bytes  which 0: the activation buffer the forward fills (and the backward reads); which 1: the
 *       backward workspace.  0 for an invalid geometry.
 *   msda_smoother_forward_f32      2 nb + 3 launches (one per depth over every Smoother of every module, then the fusions).
 *   msda_smoother_backward_f32     at most 2 nb + 5 launches: input gradients per depth (the encoders' only when some grad_x[i]
 *       is non-null), one weight-gradient launch over every layer, one fold of the pos / vel / acc adjoints onto grad_x[i]
 *       [B * T, C].  grad_params: one flat buffer, the modules' parameters concatenated in the order of `params`; every
 *       element written.  grad_x: host array (may be NULL), entries NULL where no input gradient is wanted.
 *   msda_smoother_dropout_mask_f32 (tests) the keep mask (1 / 0) of (problem, layer) over [rows, cols], from the kernels'
 *       own device function.
 * Selection: logits [bs, Q, K]; sources (HOST array of 6, fp32 contiguous): hand_cam [bs, Q, 3], obj_cam [bs, Q, 3],
 * mano_pose [bs, Q, 48], mano_shape [bs, Q, 10], obj_rad [bs, Q, 1], obj_rot [bs, Q, 3]; out (HOST array of 9): root_l,
 * root_r, root_o [bs, 3], pose_l, pose_r [bs, 48], shape_l, shape_r [bs, 10], obj_rot [bs, 3], obj_rad [bs, 1]; idx [bs, 3]
 * (left, right, object query).  The object rule runs over classes 1 .. obj_end - 1 (obj_end = cfg.hand_idx[0]).
 *   msda_arctic_item_forward_f32   one launch.  msda_arctic_item_backward_f32: one launch; writes every element of the six
 *       source gradients; grad_out entries may be NULL (no gradient).
 * Grouped selection (arctic_tools/process.py:20-70 for n_sets prediction sets of one shape, 1 <= n_sets <= 8): logits a HOST
 * array of n_sets fp32 [bs, Q, K]; sources a HOST array of n_sets * 6 (set-major, the order above), all fp32 (src_bf16 = 0) or
 * all bf16 bits (src_bf16 = 1; rows need 2-byte alignment only); out a HOST array of n_sets * 9 fp32 tensors, for bf16 sources
 * the gathered values widened exactly; idx [n_sets, bs, 3].
 *   msda_arctic_item_many_forward  one launch, grid (bs, n_sets); the rule, and for fp32 sources the bits, of
 *       msda_arctic_item_forward_f32 per set.
 *   msda_arctic_item_many_backward one launch; grad_out a HOST array of n_sets * 9 fp32 tensors (entries may be NULL);
 *       grad_sources a HOST array of n_sets * 6 tensors of the sources' dtype, every element written.  A row's gradients are
 *       summed in fp32, left hand first, and a bf16 result is rounded once, to nearest even.
 * Fixed summation order, no atomics: bitwise reproducible.  No allocation, no synchronisation; argument errors before any
 * launch. */
int msda_smoother_supported(int T, int O, int H, int R, int num_blocks);
unsigned long long msda_smoother_workspace_bytes(int T, int O, int H, int R, int num_blocks, int n_mod, int n_calls,
                                                 const int *call_mod, const int *call_B, const int *call_C, int which);
int msda_smoother_forward_f32(int T, int O, int H, int R, int num_blocks, int n_mod, int n_calls, const int *call_mod,
                              const int *call_B, const int *call_C, const float *const *x, const float *const *params,
                              float *const *out, float *act, unsigned long long act_bytes, int training, float p,
                              const unsigned long long *seed, msda_stream_t stream);
int msda_smoother_backward_f32(int T, int O, int H, int R, int num_blocks, int n_mod, int n_calls, const int *call_mod,
                               const int *call_B, const int *call_C, const float *const *x, const float *const *params,
                               const float *act, unsigned long long act_bytes, const float *const *grad_out,
                               float *const *grad_x, float *grad_params, int training, float p,
                               const unsigned long long *seed, void *workspace, unsigned long long workspace_bytes,
                               msda_stream_t stream);
int msda_smoother_dropout_mask_f32(const unsigned long long *seed, int problem, int layer, int rows, int cols, float p, float *mask,
                                   msda_stream_t stream);
int msda_arctic_item_forward_f32(int bs, int Q, int K, int obj_end, int hand_l, int hand_r, const float *logits,
                                 const float *const *sources, float *const *out, int64_t *idx, msda_stream_t stream);
int msda_arctic_item_backward_f32(int bs, int Q, const int64_t *idx, const float *const *grad_out, float *const *grad_sources,
                                  msda_stream_t stream);
int msda_arctic_item_many_forward(int n_sets, int bs, int Q, int K, int obj_end, int hand_l, int hand_r, int src_bf16,
                                  const float *const *logits, const void *const *sources, float *const *out, int64_t *idx,
                                  msda_stream_t stream);
int msda_arctic_item_many_backward(int n_sets, int bs, int Q, int src_bf16, const int64_t *idx, const float *const *grad_out,
                                   void *const *grad_sources, msda_stream_t stream);

/* ---- Swin window attention (models/swin_transformer.py:126-142 WindowAttention.forward, :210-240 SwinTransformerBlock's pad /
 * roll / partition / reverse / crop, :339-357 BasicLayer's shift mask) for head_dim 32 -----------------------------------------
 * Added after MSDA_ABI_VERSION 116 without a version bump: purely additive entries.
 *
 * Geometry: B images of H x W real tokens, C = 32 nH channels, window ws (1 <= ws <= 12), shift 0 <= shift < ws.  qkv
 * [B H W, 3 C]: the qkv Linear's output on the real tokens only, columns (3, nH, 32); qkv_bias [3 C] or NULL (no bias: padded
 * tokens' k and v are 0); table [(2 ws - 1)^2, nH] (relative_position_bias_table); out [B H W, C], columns (nH, 32).  The map
 * is padded to Hp = ceil(H / ws) ws, Wp likewise, and rolled by -shift: window position (Y, X) reads token ((Y + shift) mod Hp,
 * (X + shift) mod Wp); one outside H x W is padded (k, v = the bias's parts, its output cropped).  q is scaled by 32^-0.5; the
 * bias index and the -100 shift mask are computed from coordinates.
 *   msda_swin_attn_workspace_bytes  which 0: the lse buffer the forward fills and the backward reads; which 1: the backward
 *       workspace.  0 for an unsupported geometry.
 *   msda_swin_attn_forward_f32   one launch: out for every real token, the log-sum-exp of every real query.
 *   msda_swin_attn_backward_f32  three launches: grad_qkv [B H W, 3 C] (every element written), grad_table [(2 ws - 1)^2, nH],
 *       grad_qkv_bias [3 C] (may be NULL): the k and v gradients summed over padded tokens, q part 0 — the extra gradient of
 *       qkv.bias that the padded rows carry (autograd adds the Linear's own).
 * Fixed summation order, no atomics: bitwise reproducible.  No allocation, no synchronisation; argument errors before any
 * launch. */
int msda_swin_attn_supported(int B, int H, int W, int C, int nH, int ws, int shift);
unsigned long long msda_swin_attn_workspace_bytes(int B, int H, int W, int C, int nH, int ws, int shift, int which);
int msda_swin_attn_forward_f32(int B, int H, int W, int C, int nH, int ws, int shift, const float *qkv, const float *qkv_bias,
                               const float *table, float *out, float *lse, unsigned long long lse_bytes, msda_stream_t stream);
int msda_swin_attn_backward_f32(int B, int H, int W, int C, int nH, int ws, int shift, const float *qkv, const float *qkv_bias,
                                const float *table, const float *out, const float *lse, unsigned long long lse_bytes,
                                const float *grad_out, float *grad_qkv, float *grad_table, float *grad_qkv_bias, void *workspace,
                                unsigned long long workspace_bytes, msda_stream_t stream);

/* The bf16-autocast form of the same node.  Added after MSDA_ABI_VERSION 116 without a version bump: purely additive entries.
 * qkv, out, grad_out and grad_qkv are bf16 (uint16_t bit patterns, 16-byte aligned bases); qkv_bias, table, lse, grad_table,
 * grad_qkv_bias and the workspace stay fp32, and msda_swin_attn_supported / msda_swin_attn_workspace_bytes serve both forms
 * with the same sizes.  A padded token's k and v are the bias's parts rounded to bf16 (what a bf16 Linear gives a zero row).
 * Every product runs on the bf16 MFMA with fp32 accumulation; scores (scale, table term, shift mask), softmax, log-sum-exp,
 * delta and dP stay fp32; P and dS are rounded to bf16 only as matrix operands, out and grad_qkv once.  Same launch counts
 * (one forward, three backward), same fixed summation order, same argument checks before any launch. */
int msda_swin_attn_forward_bf16(int B, int H, int W, int C, int nH, int ws, int shift, const uint16_t *qkv, const float *qkv_bias,
                                const float *table, uint16_t *out, float *lse, unsigned long long lse_bytes, msda_stream_t stream);
int msda_swin_attn_backward_bf16(int B, int H, int W, int C, int nH, int ws, int shift, const uint16_t *qkv,
                                 const float *qkv_bias, const float *table, const uint16_t *out, const float *lse,
                                 unsigned long long lse_bytes, const uint16_t *grad_out, uint16_t *grad_qkv, float *grad_table,
                                 float *grad_qkv_bias, void *workspace, unsigned long long workspace_bytes, msda_stream_t stream);

/* ---- The Swin blocks' residual, drop-path and LayerNorm glue, and PatchMerging's gather + norm (models/swin_transformer.py:
 * 209-245 SwinTransformerBlock.forward's norm1 / shortcut + drop_path / norm2 / x + drop_path, :263-287 PatchMerging.forward) ----
 * Added after MSDA_ABI_VERSION 116 without a version bump: purely additive entries.
 *
 * Rows x and y [rows, C] are fp32 (the residual stream).  T, the suffix, is the type of the branch a [rows, C], of the drop-path
 * scale keep [ceil(rows / rows_per_sample)] (NULL: 1), of the normalised rows z and of their gradients: float (_f32) or bf16 bit
 * patterns (_bf16).  Widths: C % 4 == 0 and 0 < C <= 3072 (msda_swin_glue_supported); fp32 rows and parameters 16-byte aligned,
 * bf16 rows 8-byte; rows_per_sample > 0; 0 <= rows <= 2^32.  rnd_T rounds to bf16 (nearest even) for _bf16 and is the identity
 * for _f32; no product is contracted with the add that follows it, so y is what torch's x + a * keep gives, bit for bit.
 *   norm        forward   z = LN(x) gamma + beta; mean, rstd [rows] saved.
 *               backward  grad_x from grad_z; grad_gamma, grad_beta.
 *   add_norm    forward   y = x + rnd_T(a keep[row / rows_per_sample]), z = LN(y) gamma + beta, in one launch.
 *               backward  grad_x = grad_y + LN'(grad_z), grad_a = rnd_T(rnd_T(grad_x) keep[..]) (keep NULL: rnd_T(grad_x)) in the
 *                         same pass, from the saved y; grad_a may be NULL for _f32 without keep (it equals grad_x).
 *   add         forward   y = x + rnd_T(a keep[..]).   backward  grad_a as above from grad_y (grad_x is grad_y itself).
 *   merge_norm  x [B, H, W, C] -> z [B, ceil(H/2) ceil(W/2), 4 C] = LN over the channels of tokens (2i, 2j), (2i+1, 2j),
 *               (2i, 2j+1), (2i+1, 2j+1) in this order, zeros where an odd H or W is padded; 4 C <= 3072; gamma, beta [4 C].
 *               backward  grad_x [B, H, W, C]: every element written once.
 * Each forward is one launch; each backward with parameter gradients is two (the rows' pass, which leaves per-workgroup partial
 * column sums in the workspace, and one fixed-order reduction): no float atomics, bitwise reproducible.  add's backward is one.
 * msda_swin_glue_workspace_bytes(rows, C) = min(1024, max(1, ceil(rows / 16))) * 2 * C * 4 (0 for an unsupported width); for
 * merge_norm with rows = B ceil(H/2) ceil(W/2) and the width 4 C.  The workspace is 16-byte aligned.  No allocation, no
 * synchronisation; argument errors before any launch. */
int msda_swin_glue_supported(int C);
unsigned long long msda_swin_glue_workspace_bytes(long long rows, int C);
int msda_swin_glue_norm_forward_f32(const float *x, const float *gamma, const float *beta, long long rows, int C, float eps,
                                    float *z, float *mean, float *rstd, msda_stream_t stream);
int msda_swin_glue_norm_forward_bf16(const float *x, const float *gamma, const float *beta, long long rows, int C, float eps,
                                     uint16_t *z, float *mean, float *rstd, msda_stream_t stream);
int msda_swin_glue_norm_backward_f32(const float *grad_z, const float *x, const float *gamma, const float *mean,
                                     const float *rstd, long long rows, int C, float *grad_x, float *grad_gamma,
                                     float *grad_beta, void *workspace, unsigned long long workspace_bytes, msda_stream_t stream);
int msda_swin_glue_norm_backward_bf16(const uint16_t *grad_z, const float *x, const float *gamma, const float *mean,
                                      const float *rstd, long long rows, int C, float *grad_x, float *grad_gamma,
                                      float *grad_beta, void *workspace, unsigned long long workspace_bytes, msda_stream_t stream);
int msda_swin_glue_add_norm_forward_f32(const float *x, const float *a, const float *keep, long long rows,
                                        long long rows_per_sample, int C, const float *gamma, const float *beta, float eps,
                                        float *y, float *z, float *mean, float *rstd, msda_stream_t stream);
int msda_swin_glue_add_norm_forward_bf16(const float *x, const uint16_t *a, const uint16_t *keep, long long rows,
                                         long long rows_per_sample, int C, const float *gamma, const float *beta, float eps,
                                         float *y, uint16_t *z, float *mean, float *rstd, msda_stream_t stream);
int msda_swin_glue_add_norm_backward_f32(const float *grad_y, const float *grad_z, const float *y, const float *keep,
                                         const float *gamma, const float *mean, const float *rstd, long long rows,
                                         long long rows_per_sample, int C, float *grad_x, float *grad_a, float *grad_gamma,
                                         float *grad_beta, void *workspace, unsigned long long workspace_bytes,
                                         msda_stream_t stream);
int msda_swin_glue_add_norm_backward_bf16(const float *grad_y, const uint16_t *grad_z, const float *y, const uint16_t *keep,
                                          const float *gamma, const float *mean, const float *rstd, long long rows,
                                          long long rows_per_sample, int C, float *grad_x, uint16_t *grad_a, float *grad_gamma,
                                          float *grad_beta, void *workspace, unsigned long long workspace_bytes,
                                          msda_stream_t stream);
int msda_swin_glue_add_forward_f32(const float *x, const float *a, const float *keep, long long rows, long long rows_per_sample,
                                   int C, float *y, msda_stream_t stream);
int msda_swin_glue_add_forward_bf16(const float *x, const uint16_t *a, const uint16_t *keep, long long rows,
                                    long long rows_per_sample, int C, float *y, msda_stream_t stream);
int msda_swin_glue_add_backward_f32(const float *grad_y, const float *keep, long long rows, long long rows_per_sample, int C,
                                    float *grad_a, msda_stream_t stream);
int msda_swin_glue_add_backward_bf16(const float *grad_y, const uint16_t *keep, long long rows, long long rows_per_sample, int C,
                                     uint16_t *grad_a, msda_stream_t stream);
int msda_swin_glue_merge_norm_forward_f32(const float *x, int B, int H, int W, int C, const float *gamma, const float *beta,
                                          float eps, float *z, float *mean, float *rstd, msda_stream_t stream);
int msda_swin_glue_merge_norm_forward_bf16(const float *x, int B, int H, int W, int C, const float *gamma, const float *beta,
                                           float eps, uint16_t *z, float *mean, float *rstd, msda_stream_t stream);
int msda_swin_glue_merge_norm_backward_f32(const float *grad_z, const float *x, const float *gamma, const float *mean,
                                           const float *rstd, int B, int H, int W, int C, float *grad_x, float *grad_gamma,
                                           float *grad_beta, void *workspace, unsigned long long workspace_bytes,
                                           msda_stream_t stream);
int msda_swin_glue_merge_norm_backward_bf16(const uint16_t *grad_z, const float *x, const float *gamma, const float *mean,
                                            const float *rstd, int B, int H, int W, int C, float *grad_x, float *grad_gamma,
                                            float *grad_beta, void *workspace, unsigned long long workspace_bytes,
                                            msda_stream_t stream);

/* ---- The same glue over a bf16 residual stream (suffix <T>_sbf16, s = stream) ------------------------------------------------
 * Added after MSDA_ABI_VERSION 116 without a version bump: purely additive entries.
 *
 * Under bf16 autocast PatchMerging's reduction returns bf16, so from the second stage on the residual stream x, y and their
 * gradients are bf16 bit patterns [rows, C], 8-byte aligned.  T is bf16 for all four operations and float for norm alone (the
 * per-stage output norms).  Argument order, widths, workspace formula, launch counts and argument checks are those of the
 * fp32-stream entries above.  rnd rounds to bf16 (nearest even), LN is the fp32 LayerNorm of float(rows), LN' its backward;
 * the rounding points are those of torch's bf16 arithmetic under autocast:
 *
 *   op          forward                                               backward
 *   norm        z = rnd(LN(x))  (_f32_sbf16: z = LN(x), fp32);        grad_x = rnd(LN'(grad_z)), bf16 (the caller's autograd adds the
 *               mean, rstd fp32                                       shortcut's gradient); grad_gamma, grad_beta fp32 as above
 *   add_norm    y = rnd(float(x) + float(rnd(a keep))), bf16;         grad_x = rnd(float(grad_y) + float(rnd(LN'(grad_z)))): the cast's
 *               z = rnd(LN(y)) over the ROUNDED y, not over the       backward, then the bf16 accumulation.  grad_a = rnd(grad_x keep);
 *               fp32 sum                                              keep NULL: grad_a is grad_x, pass grad_a NULL
 *   add         y = rnd(float(x) + float(rnd(a keep)))                grad_x is grad_y itself.  grad_a = rnd(grad_y keep): one launch;
 *                                                                     keep NULL is refused (grad_a would be grad_y: nothing to compute)
 *   merge_norm  bf16 x [B, H, W, C] -> z = rnd(LN(cat)), padded       grad_x bf16 [B, H, W, C]: every real token written once
 *               positions read zero
 *
 * keep stays the caller's draw, of type T; no kernel generates random numbers; nothing is contracted into an fma; no float
 * atomics, bitwise reproducible, no allocation, no synchronisation; argument errors before any launch. */
int msda_swin_glue_norm_forward_f32_sbf16(const uint16_t *x, const float *gamma, const float *beta, long long rows, int C,
                                          float eps, float *z, float *mean, float *rstd, msda_stream_t stream);
int msda_swin_glue_norm_forward_bf16_sbf16(const uint16_t *x, const float *gamma, const float *beta, long long rows, int C,
                                           float eps, uint16_t *z, float *mean, float *rstd, msda_stream_t stream);
int msda_swin_glue_norm_backward_f32_sbf16(const float *grad_z, const uint16_t *x, const float *gamma, const float *mean,
                                           const float *rstd, long long rows, int C, uint16_t *grad_x, float *grad_gamma,
                                           float *grad_beta, void *workspace, unsigned long long workspace_bytes,
                                           msda_stream_t stream);
int msda_swin_glue_norm_backward_bf16_sbf16(const uint16_t *grad_z, const uint16_t *x, const float *gamma, const float *mean,
                                            const float *rstd, long long rows, int C, uint16_t *grad_x, float *grad_gamma,
                                            float *grad_beta, void *workspace, unsigned long long workspace_bytes,
                                            msda_stream_t stream);
int msda_swin_glue_add_norm_forward_bf16_sbf16(const uint16_t *x, const uint16_t *a, const uint16_t *keep, long long rows,
                                               long long rows_per_sample, int C, const float *gamma, const float *beta,
                                               float eps, uint16_t *y, uint16_t *z, float *mean, float *rstd,
                                               msda_stream_t stream);
int msda_swin_glue_add_norm_backward_bf16_sbf16(const uint16_t *grad_y, const uint16_t *grad_z, const uint16_t *y,
                                                const uint16_t *keep, const float *gamma, const float *mean, const float *rstd,
                                                long long rows, long long rows_per_sample, int C, uint16_t *grad_x,
                                                uint16_t *grad_a, float *grad_gamma, float *grad_beta, void *workspace,
                                                unsigned long long workspace_bytes, msda_stream_t stream);
int msda_swin_glue_add_forward_bf16_sbf16(const uint16_t *x, const uint16_t *a, const uint16_t *keep, long long rows,
                                          long long rows_per_sample, int C, uint16_t *y, msda_stream_t stream);
int msda_swin_glue_add_backward_bf16_sbf16(const uint16_t *grad_y, const uint16_t *keep, long long rows,
                                           long long rows_per_sample, int C, uint16_t *grad_a, msda_stream_t stream);
int msda_swin_glue_merge_norm_forward_bf16_sbf16(const uint16_t *x, int B, int H, int W, int C, const float *gamma,
                                                 const float *beta, float eps, uint16_t *z, float *mean, float *rstd,
                                                 msda_stream_t stream);
int msda_swin_glue_merge_norm_backward_bf16_sbf16(const uint16_t *grad_z, const uint16_t *x, const float *gamma,
                                                  const float *mean, const float *rstd, int B, int H, int W, int C,
                                                  uint16_t *grad_x, float *grad_gamma, float *grad_beta, void *workspace,
                                                  unsigned long long workspace_bytes, msda_stream_t stream);

/* ---- MANO hand layer (smplx MANO with use_pca=False: lbs = Rodrigues, shape and pose blend shapes, kinematic chain, linear
 * blend skinning) over several groups of hands -------------------------------------------------------------------------------
 * Added after MSDA_ABI_VERSION 116 without a version bump: purely additive entries.
 *
 * V vertices (1 <= V <= 8192), 16 joints, n_betas shape coefficients (1 .. 16), n_extra extra joints (0 .. 8: vertex ids).
 * n_layers <= 4 models; layer_tensors: HOST array of 7 pointers per layer, fp32 contiguous: v_template [V, 3], shapedirs
 * [V, 3, n_betas], posedirs [135, 3 V] (smplx's layout), J_template [16, 3] = J_regressor . v_template, J_shapedirs
 * [16, 3, n_betas] = J_regressor . shapedirs, lbs_weights [V, 16], pose_mean [48].  layer_index: HOST ints, 16 + n_extra per
 * layer: parents (parents[0] = -1, 0 <= parents[j] < j), then the extra-joint vertex ids.
 * n_groups <= 16 groups; group i runs layer group_layer[i] over group_B[i] >= 0 hands; group_bcast (may be NULL): nonzero = one
 * betas row for every hand.  inputs: HOST array of 4 per group: betas [B or 1, n_betas], global_orient [B, 3], hand_pose
 * [B, 45], transl [B, 3] (NULL: none).  outputs: 2 per group: vertices [B, V, 3], joints [B, 16 + n_extra, 3] (the posed
 * joints, then the extra vertices; transl added to both).
 *   msda_mano_workspace_bytes  the backward workspace; 0 for an unsupported geometry.
 *   msda_mano_forward_f32      one launch.
 *   msda_mano_backward_f32     two launches.  grad_outputs: 2 per group, g_vertices and g_joints, either may be NULL (zero).
 *       grads: 4 per group: g_betas [B, n_betas] per hand (the caller sums them for a broadcast betas row), g_global_orient
 *       [B, 3], g_hand_pose [B, 45], g_transl [B, 3] (NULL: not wanted).  No gradient of the model tensors.
 * Fixed summation order, no atomics: bitwise reproducible.  No allocation, no synchronisation; argument errors before any
 * launch. */
int msda_mano_supported(int V, int n_betas, int n_extra);
unsigned long long msda_mano_workspace_bytes(int V, int n_betas, int n_extra, int n_groups, const int *group_B);
int msda_mano_forward_f32(int V, int n_betas, int n_extra, int n_layers, const float *const *layer_tensors, const int *layer_index,
                          int n_groups, const int *group_layer, const int *group_B, const int *group_bcast,
                          const float *const *inputs, float *const *outputs, msda_stream_t stream);
int msda_mano_backward_f32(int V, int n_betas, int n_extra, int n_layers, const float *const *layer_tensors, const int *layer_index,
                           int n_groups, const int *group_layer, const int *group_B, const int *group_bcast,
                           const float *const *inputs, const float *const *grad_outputs, float *const *grads, void *workspace,
                           unsigned long long workspace_bytes, msda_stream_t stream);

/* ---- ARCTIC object layer and small losses (csrc/msda_small_loss.hip) ------------------------------------------------------------
 * Added after MSDA_ABI_VERSION 116 without a version bump: purely additive entries.
 *
 * Object layer (arctic_tools ObjectTensors.forward_7d_batch).  dims: HOST ints {n_objects (1 .. 64), Lm padded template rows
 * (1 .. 65536), NS sub-vertices (0 .. 4096), NBt, NBb bbox corners (sum <= 64), NKt, NKb keypoints (sum <= 256)}.  model: HOST
 * array of 8 device pointers: v [N, Lm, 3] f32, parts_ids [N, Lm] int64, v_sub [N, NS, 3] f32, parts_sub_ids [N, NS] int64,
 * bbox_top [N, NBt, 3], bbox_bottom [N, NBb, 3], kp_top [N, NKt, 3], kp_bottom [N, NKb, 3] (f32; metres).  n_groups <= 16;
 * group i has group_B[i] >= 0 frames and group_len[i] (1 .. Lm) output template rows.  inputs: 4 per group: obj_idx [B] int64,
 * angles [B], global_orient [B, 3], transl [B, 3] (NULL: none).  outputs: 4 per group: v [B, len, 3], v_sub [B, NS, 3], bbox3d
 * [B, NBt + NBb, 3], kp3d [B, NKt + NKb, 3] (top rows first).  An obj_idx outside 0 .. N - 1 gives NaN rows.
 *   msda_object_forward_f32   one launch.
 *   msda_object_backward_f32  one launch.  grad_outputs: 4 per group (NULL: zero); grads: 3 per group: g_angles [B],
 *       g_global_orient [B, 3], g_transl [B, 3] (each NULL: not wanted).
 *
 * Small losses (compute_small_loss) of S sets (1 .. 8) over B frames.  dims: HOST ints {S, B, J hand joints (1 .. 32), NV hand
 * vertices (1 .. 1024), KO object keypoints (even, 2 .. 64), NB betas (1 .. 16), L object rows (1 .. 65536)}.  targets: HOST
 * array of 25 device pointers, fp32 contiguous unless noted: mano.pose.l [B, 48], mano.pose.r, mano.beta.l [B, NB],
 * mano.beta.r, mano.j3d.cam.l [B, J, 3], mano.j3d.cam.r, object.kp3d.cam [B, KO, 3], mano.j2d.norm.l [B, J, 2], mano.j2d.norm.r,
 * object kp2d (norm.t then norm.b) [B, KO, 2], object.rot [B, 3], object.radian [B], mano.cam_t.wp.l [B, 3], mano.cam_t.wp.r,
 * object.cam_t.wp, is_valid [B], left_valid [B], right_valid [B], joints_valid_l [B, J], joints_valid_r, dist.ro [B, NV],
 * dist.lo, intrinsics [B, 3, 3], idx.ro [B, NV] int64, idx.lo.  inputs: HOST array of 15 per set: root_l, root_r, root_o
 * [B, 3], pose_l, pose_r [B, 48], betas_l, betas_r [B, NB], rot [B, 3], radian [B], MANO vertices l, r [B, NV, 3] and joints
 * l, r [B, J, 3] (no camera translation), object v [B, L, 3] and kp3d [B, KO, 3].  losses: [S, 19] in compute_small_loss's
 * key order.
 *   msda_small_loss_workspace_bytes  the forward's workspace, which the backward reads; 0 for an unsupported geometry.
 *   msda_small_loss_forward_f32      two launches (none for B = 0: the losses are then left unwritten).
 *   msda_small_loss_backward_f32     one launch.  grad_losses [S, 19]; grads: 15 per set, shaped as the inputs.
 * Fixed summation order, no atomics: bitwise reproducible.  No allocation, no synchronisation; argument errors before any
 * launch. */
int msda_object_supported(int n_objects, int max_len, int n_sub, int n_bbox_top, int n_bbox_bottom, int n_kp_top, int n_kp_bottom);
int msda_object_forward_f32(const int *dims, const void *const *model, int n_groups, const int *group_B, const int *group_len,
                            const void *const *inputs, float *const *outputs, msda_stream_t stream);
int msda_object_backward_f32(const int *dims, const void *const *model, int n_groups, const int *group_B, const int *group_len,
                             const void *const *inputs, const float *const *grad_outputs, float *const *grads,
                             msda_stream_t stream);
int msda_small_loss_supported(int S, int B, int J, int NV, int KO, int NB, int L);
unsigned long long msda_small_loss_workspace_bytes(int S, int B, int J, int NV, int KO, int NB, int L);
int msda_small_loss_forward_f32(const int *dims, float img_res, const void *const *targets, const float *const *inputs,
                                float *losses, void *workspace, unsigned long long workspace_bytes, msda_stream_t stream);
int msda_small_loss_backward_f32(const int *dims, float img_res, const void *const *targets, const float *const *inputs,
                                 const float *grad_losses, float *const *grads, const void *workspace,
                                 unsigned long long workspace_bytes, msda_stream_t stream);

/* ---- ARCTIC evaluation: nearest neighbour and metrics (csrc/msda_arctic_eval.hip) ------------------------------------------------
 * Added after MSDA_ABI_VERSION 116 without a version bump: purely additive entries.
 *
 * Nearest neighbour (arctic_tools/src/utils/loss_modules.py get_NN, i.e. pytorch3d knn_points with K = 1 and full lengths).
 * n_pairs (1 .. 8) pairs share B (0 .. 65535), N1 (1 .. 8192) and N2 (1 .. 1024).  src, trg: HOST arrays of n_pairs device
 * pointers, src [B, N1, 3], trg [B, N2, 3], fp32 contiguous.  dists [B, N1] fp32: the SQUARED distance to the nearest target,
 * dx dx + dy dy + dz dz summed in that order; idx [B, N1] int64.  The minimum moves on strict < only: the lowest index wins a
 * tie, a NaN distance never wins (no finite candidate: +inf, index 0).
 *   msda_nn_supported     1 when the kernels take this geometry.
 *   msda_nn_forward_f32   one launch (none for B = 0).
 *   msda_nn_backward_f32  one launch.  grad_dists [B, N1]; grad_src [B, N1, 3] = 2 g (a - b_idx), grad_trg [B, N2, 3] =
 *       -sum over the sources with idx == j, in source order without atomics (bitwise reproducible); either output pointer
 *       may be NULL (not wanted).  An idx outside 0 .. N2 - 1 contributes nothing.
 *
 * Metrics (arctic_tools/process.py measure_error over src/utils/eval_modules.py eval_degree, eval_mpjpe_ra, eval_mrrpe,
 * eval_v2v_success, eval_contact_deviation and common/metrics.py).  dims: HOST ints {B frames, J hand joints (1 .. 32), NV hand
 * vertices (1 .. 1024), L_pred rows of pred object.v.cam, L_gt rows of targets object.v.cam, L_parts rows of part_ids (each
 * 1 .. 65536)}.  floats: HOST array of 16 device pointers, fp32 contiguous: pred object.radian [B], targets object.radian [B],
 * pred mano.j3d.cam.r, pred mano.j3d.cam.l, targets mano.j3d.cam.r, targets mano.j3d.cam.l [B, J, 3], pred object.v.cam
 * [B, L_pred, 3], targets object.v.cam [B, L_gt, 3], diameter [B], is_valid, left_valid, right_valid [B], pred mano.v3d.cam.r,
 * pred mano.v3d.cam.l [B, NV, 3], targets dist.ro, dist.lo [B, NV].  longs: HOST array of 4 device pointers, int64: object.v_len
 * [B], part_ids [B, L_parts], idx.ro, idx.lo [B, NV].  out [6, B]: aae (degrees), mpjpe/ra/h, mrrpe/r/l, mrrpe/r/o (mm),
 * success_rate/0.05 (percent), cdev/ho (mm); NaN where the reference has NaN.
 *   msda_arctic_metrics_f32             one launch, one workgroup per frame, fixed reduction order.
 *   msda_arctic_metrics_accumulate_f32  engine.py test_pose's per-key step mean and MetricLogger.update: per key the mean over
 *       the non-NaN frames of values [6, B]; where one exists it is added to total[key] and 1 to count[key] (fp64 device arrays
 *       of 6).  One launch of one workgroup.
 * No allocation, no synchronisation; argument errors before any launch. */
int msda_nn_supported(int B, int N1, int N2);
int msda_nn_forward_f32(int n_pairs, int B, int N1, int N2, const float *const *src, const float *const *trg, float *const *dists,
                        long long *const *idx, msda_stream_t stream);
int msda_nn_backward_f32(int n_pairs, int B, int N1, int N2, const float *const *src, const float *const *trg,
                         const long long *const *idx, const float *const *grad_dists, float *const *grad_src,
                         float *const *grad_trg, msda_stream_t stream);
int msda_arctic_metrics_supported(int B, int J, int NV, int L_pred, int L_gt, int L_parts);
int msda_arctic_metrics_f32(const int *dims, const float *const *floats, const long long *const *longs, float *out,
                            msda_stream_t stream);
int msda_arctic_metrics_accumulate_f32(const float *values, int B, double *total, double *count, msda_stream_t stream);

/* ---- the input-projection neck: conv bias + GroupNorm + feature mask (csrc/msda_neck.hip) ----------------------------------------
 * Added after MSDA_ABI_VERSION 116 without a version bump: purely additive entries.
 *
 * The input_proj loop of DeformableDETR.forward (models/actic_detr.py:191-225, models/assembly_detr.py:145-171) after the
 * convolution: per feature level l,  out_l = GroupNorm(groups, C)(y_l + bias_l) * (uniform_l > 0.3f),  where y_l [N, C, H_l, W_l]
 * is the Conv2d output taken WITHOUT its bias.  Every table is a HOST array of L (1 .. 8) device pointers to fp32 contiguous
 * tensors: bias_l, gamma_l, beta_l [C]; uniform_l, out_l of y_l's shape; mean_l, rstd_l [N, groups]; mask_l one byte per
 * element of y_l (1 = kept).  heights, widths: HOST ints.  The bias table or single entries of it may be NULL (a conv without
 * bias); the uniform table may be NULL: no mask factor, mask is not touched.  The statistics are nn.GroupNorm's (biased
 * variance, eps inside the root), the variance is the centred sum of (x - mean)^2.
 *   msda_neck_supported        1 when the kernels take this geometry: C a multiple of groups, any H_l * W_l >= 1.
 *   msda_neck_workspace_bytes  scratch of the backward: 3 [N, C] fp32 partials per level.
 *   msda_neck_forward_f32      one launch for all levels (none for N = 0); writes out, mean, rstd and, with uniforms, mask.
 *   msda_neck_backward_f32     two launches.  With g' = grad_out * mask and x^ = (y + bias - mean) rstd per (frame, group):
 *       grad_y = rstd (g' gamma - mean_grp(g' gamma) - x^ mean_grp(g' gamma x^)); grad_gamma = sum g' x^, grad_beta = sum g',
 *       grad_bias = sum grad_y over frames and pixels (each table or entry may be NULL: not wanted).  mask table NULL: no mask.
 * Every sum runs in a fixed order without atomics: all results are bitwise reproducible.  No allocation, no
 * synchronisation; argument errors before any launch. */
int msda_neck_supported(int L, int N, int C, int groups, const int *heights, const int *widths);
unsigned long long msda_neck_workspace_bytes(int L, int N, int C);
int msda_neck_forward_f32(int L, const float *const *y, const float *const *bias, const float *const *gamma,
                          const float *const *beta, const float *const *uniform, const int *heights, const int *widths, int N, int C,
                          int groups, float eps, float *const *out, float *const *mean, float *const *rstd,
                          unsigned char *const *mask, msda_stream_t stream);
int msda_neck_backward_f32(int L, const float *const *grad_out, const float *const *y, const float *const *bias,
                           const float *const *gamma, const float *const *mean, const float *const *rstd,
                           const unsigned char *const *mask, const int *heights, const int *widths, int N, int C, int groups,
                           float *const *grad_y, float *const *grad_gamma, float *const *grad_beta, float *const *grad_bias,
                           void *workspace, unsigned long long workspace_bytes, msda_stream_t stream);

/* ---- make_output's pose, camera and projection glue (csrc/msda_arctic_output.hip) --------------------------------------------------
 * Added after MSDA_ABI_VERSION 116 without a version bump: purely additive entries.
 *
 * What runs between get_arctic_item, the MANO / object layers and get_NN in arctic_tools/process.py make_output (107-149) and
 * prepare_data (249-299).  Every table is a HOST array of device pointers to fp32 contiguous tensors; B = 0 .. 65535 frames.
 *
 * Pose heads.  Replaces make_output's axis_angle_to_matrix (process.py:118-119), MANOHead.forward's matrix_to_axis_angle
 * (src/nets/hand_heads/mano_head.py:30, common/rot.py:180) for n_hands (0 .. 2) poses [B, 48], and the
 * weak_perspective_to_perspective_torch calls of MANOHead / ArtiHead (mano_head.py:40, src/nets/obj_heads/obj_head.py:39) for
 * n_roots (0 .. 3) roots [B, 3] with K [B, 3, 3] (f = (K00 + K11) / 2).
 *   msda_arctic_pose_supported     1 when the kernels take this geometry (n_hands + n_roots >= 1).
 *   msda_arctic_pose_forward_f32   one launch, one thread per (hand, frame, joint) and per (root, frame): mats [B, 16, 3, 3]
 *       (pytorch3d's quaternion route, 1/2 - theta^2/48 below 1e-6), aa [B, 48] (x > 0 before the root, 2 max(|q|, 0.1), the
 *       largest |q| with the lowest index on a tie, atan2, the polynomial below 1e-6), cam_t [B, 3] = (tx, ty,
 *       2 f / (img_res max(s, 0.1) + 1e-9)).
 *   msda_arctic_pose_backward_f32  one launch.  grad_mats / grad_aa / grad_cam_t entries may be NULL (zero); grad_poses /
 *       grad_roots entries may be NULL (not wanted).  The chosen candidate and the branches are constants; the clamps pass the
 *       gradient at equality as torch.clamp does; K has no gradient.
 *
 * Matrix to axis-angle.  Replaces prepare_data's overwrite of mano.pose.r / .l (process.py:275-280) for n_hands (1 .. 2) given
 * mats [B, 16, 3, 3] -> aa [B, 16, 3]: the second half of the pose heads, forward and backward one launch each.
 *
 * Place and project.  Replaces the `+ cam_t[:, None, :]` translations and project2d + normalisation of MANOHead / ArtiHead
 * (mano_head.py:44-47, obj_head.py:44-49 and :74) and prepare_data's unormalize_kp2d of the prediction
 * (process.py:266-268).  n_segments (1 .. 8) segments; rows, camera, project: HOST ints per segment (1 .. 8192 rows, camera
 * 0 .. 2, project 0 / 1); points [B, rows, 3]; cam_t: HOST array of 3 device pointers [B, 3] (an unused camera may be NULL).
 *   msda_arctic_place_supported    1 when the kernels take n_segments segments of at most max_rows rows.
 *   msda_arctic_place_forward_f32  one launch: placed = points + cam_t (padded rows like any other); for projected segments
 *       norm2d [B, rows, 2] = 2 (K x)_xy / (K x)_z / img_res - 1 and pix2d = 0.5 img_res (norm2d + 1); their entries may be
 *       NULL for the other segments.
 *   msda_arctic_place_backward_f32 one launch: the blocks that own rows write grad_points, one more block per (camera, frame)
 *       sums that camera's rows of all its segments in a fixed order into grad_cam_t [B, 3].  grad_placed / grad_norm2d /
 *       grad_pix2d entries may be NULL (zero); grad_points / grad_cam_t entries may be NULL (not wanted).  K has no gradient.
 * fp32, no atomics, fixed summation order: bitwise reproducible.  No allocation, no synchronisation; argument errors before
 * any launch; B = 0 launches nothing. */
int msda_arctic_pose_supported(int n_hands, int n_roots, int B);
int msda_arctic_pose_forward_f32(int n_hands, int n_roots, int B, float img_res, const float *const *poses,
                                 const float *const *roots, const float *K, float *const *mats, float *const *aa,
                                 float *const *cam_t, msda_stream_t stream);
int msda_arctic_pose_backward_f32(int n_hands, int n_roots, int B, float img_res, const float *const *poses,
                                  const float *const *roots, const float *K, const float *const *grad_mats,
                                  const float *const *grad_aa, const float *const *grad_cam_t, float *const *grad_poses,
                                  float *const *grad_roots, msda_stream_t stream);
int msda_arctic_m2aa_forward_f32(int n_hands, int B, const float *const *mats, float *const *aa, msda_stream_t stream);
int msda_arctic_m2aa_backward_f32(int n_hands, int B, const float *const *mats, const float *const *grad_aa,
                                  float *const *grad_mats, msda_stream_t stream);
int msda_arctic_place_supported(int n_segments, int B, int max_rows);
int msda_arctic_place_forward_f32(int n_segments, int B, float img_res, const int *rows, const int *camera, const int *project,
                                  const float *const *points, const float *const *cam_t, const float *K, float *const *placed,
                                  float *const *norm2d, float *const *pix2d, msda_stream_t stream);
int msda_arctic_place_backward_f32(int n_segments, int B, float img_res, const int *rows, const int *camera, const int *project,
                                   const float *const *points, const float *const *cam_t, const float *K,
                                   const float *const *grad_placed, const float *const *grad_norm2d,
                                   const float *const *grad_pix2d, float *const *grad_points, float *const *grad_cam_t,
                                   msda_stream_t stream);

/* ---- the SmoothNet criterion: contact deviation and acceleration errors (csrc/msda_smooth_loss.hip) ------------------------------
 * Added after MSDA_ABI_VERSION 116 without a version bump: purely additive entries.
 *
 * compute_smoothnet_loss (arctic_tools/src/callbacks/loss/loss_arctic_sf.py:402-548): `loss/cd` of compute_contact_devi_loss
 * (src/utils/loss_modules.py:186-226) and `acc/h`, `acc/o` of eval_acc_pose / compute_error_accel
 * (src/utils/eval_modules.py:254-368) over N frames.  dims: HOST ints (N, NV, J, L): frames, hand vertices, hand joints, padded
 * object rows.  floats: HOST array of 15 device pointers to fp32 contiguous tensors, in this order: the prediction's
 * mano.v3d.cam.r, .l [N, NV, 3], mano.j3d.cam.r, .l [N, J, 3], object.v.cam [N, L, 3]; the same five of the targets; dist.ro,
 * dist.lo [N, NV]; is_valid, left_valid, right_valid [N].  longs: 3 device pointers to int64 tensors: idx.ro, idx.lo [N, NV],
 * object.parts_ids [N, L] (row 0 names the bottom columns, == 2, of every frame).  fps: the stencil is [1, -2, 1] fps^2.
 *   msda_smooth_loss_supported        1 when the kernels take this geometry: N 1 .. 8192, NV 1 .. 1024, J 1 .. 64,
 *       L 1 .. 65536.  Any number of bottom columns (none: the object terms are NaN-gated away, as in torch).
 *   msda_smooth_loss_workspace_bytes  the workspace of a forward call, which its backward call reads (0: unsupported): 6 N
 *       doubles (the object roots of prediction and gt) followed by 10 N + 4 floats.  It must be 8-byte aligned.
 *   msda_smooth_loss_forward_f32      three launches whatever the data holds.  losses [3] = loss/cd, acc/h, acc/o; frames
 *       (may be NULL) [2, N]: eval_acc_pose's acc/h [N] (NaN at both ends and where no hand counts) and acc/o [N - 2] (then
 *       padding).  A centre frame t counts iff the validity product at t - 1, t, t + 1 sums (fp64) to 3 after truncation to
 *       int64; the contact deviation counts a frame iff valid * is_valid == 1 and a vertex iff dist <= 3e-3 (a NaN distance
 *       or an index outside 0 .. L - 1 is left out as nanmean leaves a NaN out).  No counted frame: 0.
 *   msda_smooth_loss_backward_f32     one launch.  grad_losses [3]; grads: HOST array of 5 device pointers shaped as the
 *       prediction's five tensors, all written in full; acc_grad = 0 writes the contact gradient only and the two joint
 *       entries may be NULL.  A zero acceleration difference has a zero gradient.
 * fp32 inputs, outputs and arithmetic with two exceptions: the object root, a mean of coordinates at the camera's depth whose
 * fp32 rounding the stencil would multiply by fps^2, is summed, stored and subtracted in fp64 (x - root is then rounded to fp32
 * once), and the validity sum is fp64 as numpy's.  A NaN or infinite validity flag never counts.  No atomics, fixed summation
 * order: bitwise reproducible.  No allocation, no synchronisation; argument errors before any launch. */
int msda_smooth_loss_supported(int N, int NV, int J, int L);
unsigned long long msda_smooth_loss_workspace_bytes(int N, int NV, int J, int L);
int msda_smooth_loss_forward_f32(const int *dims, float fps, const float *const *floats, const long long *const *longs,
                                 float *losses, float *frames, void *workspace, unsigned long long workspace_bytes,
                                 msda_stream_t stream);
int msda_smooth_loss_backward_f32(const int *dims, float fps, const float *const *floats, const long long *const *longs,
                                  const float *grad_losses, int acc_grad, float *const *grads, const void *workspace,
                                  unsigned long long workspace_bytes, msda_stream_t stream);

/* ---- ARCTIC target preparation: rigid fit, camera translation and distance fields (csrc/msda_pre_process.hip) -----------------
 * Added after MSDA_ABI_VERSION 116 without a version bump: purely additive entries.
 *
 * Target fit: what arctic_tools/src/callbacks/process/process_arctic.py process_data (38-124) computes between its object and
 * MANO forwards and its vertex sums: common/transforms.py batch_solve_rigid_tf and rigid_tf_torch_batch (both hands), the
 * Tr0 / Tl0 means, common/data_utils.py unormalize_kp2d, common/camera.py estimate_translation_k (use_all_joints, pad_2d:
 * unit weights) over estimate_translation_k_np, and the three perspective_to_weak_perspective_torch.  B frames (>= 0), NK
 * keypoints (3 .. 64), J hand joints (1 .. 32).  inputs: HOST array of 8 device pointers, fp32 contiguous: object.kp3d.full.b
 * [B, NK, 3], the posed object's bottom kp3d without translation [B, NK, 3], object.kp2d.norm.b [B, NK, 2], intrinsics
 * [B, 3, 3], mano.j3d.full.r, .l [B, J, 3], the MANO joints r, l without translation [B, J, 3].  img_res: process_data's 224.
 * outputs: HOST array of 12 device pointers: R0 [B, 3, 3], T0 [B, 3], transl [B, 3], mano.j3d.cam.r, .l [B, J, 3], mano.cam_t.r,
 * .l [B, 3], mano.cam_t.wp.r, .l and object.cam_t.wp [B, 3], and the vertex offsets Tr0 + transl, Tl0 + transl [B, 3].
 * status [B] int32, bits: 1 the fit had a negative determinant (the reference raises; the corrected rotation of Arun's
 * method is returned), 2 the rotation is not unique (second singular value of H below 1e-6 of the first), 4 a non-finite
 * input (the frame's outputs are NaN, no other bit), 8 a singular normal matrix (transl and what depends on it are NaN).  A
 * rank-deficient H (third singular value below 1e-12 of the first: planar keypoints) has no orientation and never sets bit 1.
 * The 3 x 3 algebra runs in fp64 in a fixed order and every output is rounded to fp32 once; no frame influences another.
 *   msda_pre_fit_supported  1 when the kernel takes this geometry.
 *   msda_pre_fit_f32        one launch, one wavefront per frame (none for B = 0).
 *
 * Distance fields: arctic_tools/src/utils/interfield.py compute_dist_mano_to_obj and compute_dist_obj_to_mano as
 * src/callbacks/process/process_generic.py prepare_interfield (97-138) calls them, i.e. pytorch3d knn_points with K = 1 and
 * lengths on the object.  hand_r, hand_l [B, NV, 3], obj [B, L, 3] fp32, v_len [B] int64 (device, clamped to 0 .. L).  dists,
 * idx: HOST arrays of 4 device pointers in the order ro, lo [B, NV], or, ol [B, L]; fp32 and int64.  d = dx dx + dy dy + dz dz
 * summed in that order; the minimum moves on strict < only (lowest index on a tie, a NaN distance never wins; no finite
 * candidate: +inf, index 0); the value is clamp(sqrt(d), dist_min, dist_max).  Object rows at or beyond v_len are never
 * candidates; as sources they get 0 before the clamp and index 0, and so does every hand vertex of a frame with v_len = 0.
 *   msda_dist_fields_supported  1 when the kernel takes this geometry: B >= 0, NV 1 .. 1024, L 1 .. 65536.
 *   msda_dist_fields_f32        one launch for the four fields (none for B = 0).
 * Forward only.  No atomics: bitwise reproducible.  No allocation, no synchronisation; argument errors before any launch. */
int msda_pre_fit_supported(int B, int NK, int J);
int msda_pre_fit_f32(int B, int NK, int J, float img_res, const float *const *inputs, float *const *outputs, int *status,
                     msda_stream_t stream);
int msda_dist_fields_supported(int B, int NV, int L);
int msda_dist_fields_f32(int B, int NV, int L, const float *hand_r, const float *hand_l, const float *obj, const long long *v_len,
                         float dist_min, float dist_max, float *const *dists, long long *const *idx, msda_stream_t stream);

/* ---- The tail of the training step: gradient norm, clip and AdamW as multi-tensor launches (csrc/msda_optim.hip) ---------------
 * Added after MSDA_ABI_VERSION 116 without a version bump: purely additive entries.
 *
 * What engine.py:644-648 runs after losses.backward(): torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm) (or, for
 * max_norm <= 0, util/misc.py's get_total_grad_norm: the norm alone) and optimizer.step() of util/settings.py:434's
 * torch.optim.AdamW over three parameter groups.  fp32 only.  The number of launches does not grow with the number of tensors:
 * every tensor is cut into chunks of msda_optim_chunk_elems() elements, one workgroup per chunk, a chunk never spans two
 * tensors.  The tensors are described by DEVICE arrays that the caller owns, one entry per tensor: g, p, exp_avg, exp_avg_sq
 * (device pointers to contiguous fp32 data that need only be 4-byte aligned: a chunk moves 16-byte vectors when all its bases
 * are 16-byte aligned and single elements otherwise, with the same element-to-thread assignment, so no result depends on the
 * alignment), numel (int64), chunk_start (int64, n_tensors + 1 entries, as msda_optim_chunks lays them out), group (int32, the
 * tensor's parameter group, clamped to 0 .. n_groups - 1) and step_offset (int64).  An empty tensor owns no chunk.
 *   msda_optim_supported       1 for 0 .. 2^20 tensors in 1 .. 8 groups.
 *   msda_optim_chunk_elems     elements of a chunk.
 *   msda_optim_chunks          host logic: fills the HOST array chunk_start [n_tensors + 1] from the HOST array numel
 *       (chunk_start[i + 1] - chunk_start[i] = ceil(numel[i] / chunk)) and returns chunk_start[n_tensors], the grid size of the
 *       three chunked launches; -1 (message in msda_last_error) for a null pointer, a negative count or numel, a numel beyond
 *       2^46 or more than 2^31 - 1 chunks.
 *   msda_grad_sumsq_f32        one launch: partials [n_chunks] fp32, the sum of squares of each chunk; a thread adds its
 *       elements in index order, the workgroup its threads in a fixed tree order.
 *   msda_grad_norm_finish_f32  one launch, one workgroup: adds the partials in a fixed order (fp64, rounded once) and writes
 *       out[0] = total_norm = sqrt of the sum and out[1] = the clip coefficient exactly as torch forms it in fp32,
 *       clamp(reciprocal(total_norm + 1e-6) * max_norm, max = 1): an infinite norm gives 0, a NaN norm gives NaN.
 *       max_norm <= 0 writes the coefficient 1 (get_total_grad_norm's branch).  n_chunks = 0 launches nothing and leaves out
 *       alone (the norm of nothing is 0).
 *   msda_grad_scale_f32        one launch: g *= *coef in place (coef: device, e.g. out + 1): clip_grad_norm_ on its own.
 *   msda_adamw_step_f32        one launch.  Per element, in torch's operation order (torch/optim/adamw.py, the single-tensor
 *       form): g' = g * *coef (coef: device pointer; NULL: no clipping; g itself is never written), p *= 1 - lr wd,
 *       m += (g' - m) (1 - b1), v = v b2 + g' g' (1 - b2), p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps), with
 *       bc = 1 - beta^t evaluated in fp64 (fp32 pow loses four digits of 1 - 0.999^1) and lr / bc1, sqrt(bc2), 1 - lr wd,
 *       1 - beta rounded to fp32 once, as torch's Python scalars are.  t = global_step - step_offset[tensor] (at least 1):
 *       torch skips a parameter whose .grad is None and its step does not advance, so t is per tensor.  lr, weight_decay,
 *       beta1, beta2, eps: HOST arrays of n_groups doubles, carried by value in the kernel arguments.  Correctly rounded
 *       sqrt and division, no fast intrinsic.
 * A clipped step is sumsq + finish + step = 3 launches, an unclipped step 1; n_tensors = 0 or n_chunks = 0 launches nothing.
 * No float atomics, fixed summation order: bitwise reproducible.  No allocation, no synchronisation.  Argument errors
 * (MSDA_ERR_ARGUMENT before any launch, msda_launch_count unchanged): a null table with something to launch, a negative or
 * too large count, n_groups outside 1 .. 8, a beta outside [0, 1), a non-finite lr, eps or weight_decay, a NaN max_norm,
 * global_step < 1. */
int msda_optim_supported(long long n_tensors, int n_groups);
int msda_optim_chunk_elems(void);
long long msda_optim_chunks(int n_tensors, const long long *numel, long long *chunk_start);
int msda_grad_sumsq_f32(int n_tensors, long long n_chunks, const float *const *g, const long long *numel,
                        const long long *chunk_start, float *partials, msda_stream_t stream);
int msda_grad_norm_finish_f32(long long n_chunks, const float *partials, float max_norm, float *out, msda_stream_t stream);
int msda_grad_scale_f32(int n_tensors, long long n_chunks, float *const *g, const long long *numel, const long long *chunk_start,
                        const float *coef, msda_stream_t stream);
int msda_adamw_step_f32(int n_tensors, long long n_chunks, float *const *p, const float *const *g, float *const *exp_avg,
                        float *const *exp_avg_sq, const long long *numel, const long long *chunk_start, const int *group,
                        const long long *step_offset, int n_groups, const double *lr, const double *weight_decay,
                        const double *beta1, const double *beta2, const double *eps, long long global_step, const float *coef,
                        msda_stream_t stream);

/* The device-state forms of the same tail (engine.py:644-648: clip_grad_norm_ then optimizer.step(); util/settings.py:434-440:
 * AdamW under OneCycleLR, whose default cycle_momentum moves lr and beta1 after every step).  Added without a version bump: purely
 * additive.  They are what torch.optim.AdamW(capturable=True) needs to run inside a HIP graph: nothing that changes from step to
 * step is a kernel argument, so a captured launch replays with the values of the replay.
 *   step    DEVICE table [n_tensors] of pointers to 0-d fp32 DEVICE tensors, the state capturable=True keeps per parameter.
 *   hyper   DEVICE table [n_groups][5] of doubles: lr, weight_decay, beta1, beta2, eps of each group.  The caller validates the
 *           values (the library cannot read them without a synchronisation).
 *   msda_optim_advance_f32 (engine.py:644-648, util/settings.py:434-440)  one launch: *step[i] += 1 for every i < n_tensors; the
 *       first launch of an unclipped step.
 *   msda_grad_norm_finish_dev_f32 (engine.py:644-648, util/settings.py:434-440)  msda_grad_norm_finish_f32, then status[0] =
 *       skipped = skip_nonfinite && !isfinite(total_norm), status[1] += skipped (status: DEVICE int32 [2]; may be NULL when
 *       skip_nonfinite is 0) and, unless skipped, *step[i] += 1 for every i < n_tensors.  One launch, one workgroup.  n_tensors = 0
 *       or n_chunks = 0 launches nothing (advance the steps of tensors that are all empty with msda_optim_advance_f32).
 *   msda_adamw_step_dev_f32 (engine.py:644-648, util/settings.py:434-440)  msda_adamw_step_f32 with t = (long long)*step[tensor]
 *       (already advanced for this launch; at least 1) and decay, 1 - beta1, beta2, 1 - beta2, eps, lr / bc1, sqrt(bc2) formed on
 *       the device by the same fp64 expressions, each rounded to fp32 once: with the same values the result is bit for bit that of
 *       msda_adamw_step_f32.  coef: as there.  skip: DEVICE int32 or NULL; when *skip != 0 every workgroup returns before it reads
 *       or writes anything (pass status of the finish launch).
 * A clipped step is sumsq + finish_dev + step_dev = 3 launches, an unclipped one advance + step_dev = 2.  No float atomics, no
 * allocation, no synchronisation.  Argument errors (MSDA_ERR_ARGUMENT before any launch, msda_launch_count unchanged): counts
 * outside msda_optim_supported, a null table with something to launch, a null hyper or step table, a NaN max_norm, and a null
 * status with skip_nonfinite set. */
int msda_optim_advance_f32(int n_tensors, float *const *step, msda_stream_t stream);
int msda_grad_norm_finish_dev_f32(long long n_chunks, const float *partials, float max_norm, float *out, int n_tensors,
                                  float *const *step, int skip_nonfinite, int *status, msda_stream_t stream);
int msda_adamw_step_dev_f32(int n_tensors, long long n_chunks, float *const *p, const float *const *g, float *const *exp_avg,
                            float *const *exp_avg_sq, const long long *numel, const long long *chunk_start, const int *group,
                            const float *const *step, int n_groups, const double *hyper, const float *coef, const int *skip,
                            msda_stream_t stream);

/* Library/ABI version (major*100 + minor) and the kernel family a geometry maps to.  MSDA_ABI_VERSION is what a binding
 * compiled against THIS header expects msda_version() to return at run time (uvhand_amd/_ext.py compares the two);
 * it changes whenever a declaration in this file does.  116: msda_attn32_forward_bf16 / msda_attn32_backward_bf16 and
 * msda_add_layernorm_{forward,backward}_f32_bf16res (the bf16-autocast forms of the attention core and add + LayerNorm). */
#define MSDA_ABI_VERSION 116
int msda_version(void);
int msda_path_for(int elem_bytes, int M, int D, int L, int P);

/* Diagnostics (tests, bench, tools/ktime.py --sweep): which launch plan a call of this geometry takes, as text, e.g.
 * "fwd=lds(chunks=2,qw=528,...) bwd=fused_lds(acc=wide,W=2,...)" — the same host-side plan functions the launchers run,
 * nothing is launched.  row_bytes 4 (fp32 rows) or 2 (bf16 rows; grad_value_bytes then 2 or 4); flags as for
 * msda_backward_workspace_bytes (MSDA_FLAG_PROLOGUE: the fused-prologue entry points; has_workspace: whether the caller
 * passes the scratch that call can use).  "generic" outside the D = 32 family.  Returns the length written (NUL-terminated,
 * truncated to buf_len - 1).  No reference counterpart: the reference's dispatch is the switch over `channels` at
 * models/ops/src/cuda/ms_deform_im2col_cuda.cuh:971-1320. */
int msda_describe_plan(int row_bytes, int grad_value_bytes, int N, int S, int M, int D, int L, int Lq, int P, unsigned flags,
                       int has_workspace, char *buf, int buf_len);

/* Measurement helper (bench.py `roofline.secondary`): gathers pseudo-random rows of `table` (row_bytes 128 = fp32 rows as 8 lanes
 * x 16 B, or 64 = bf16 rows as 8 lanes x 8 B; the largest power-of-two row count that fits table_bytes) with the access
 * pattern of the sampling kernels — independent 8-lane row requests, sixteen in flight per lane — and nothing else:
 * *rows_gathered / elapsed time is the row-request rate the vector memory path of this box delivers on a table of that size,
 * the practical ceiling of a gather kernel on cache-resident data.  `sink`: one float the kernel never writes for a finite
 * table.  `blocks` x 256 threads, `iters` x 16 rows per 8-lane group.  No reference counterpart; no product path calls it. */
int msda_probe_row_gather(const void *table, unsigned long long table_bytes, int row_bytes, int blocks, int iters, float *sink,
                          unsigned long long *rows_gathered, msda_stream_t stream);

/* Diagnostic: kernel launches this process has enqueued through the library so far (one count per launcher call that reached
 * the device; a monotonically increasing relaxed atomic — the only process-wide state the library keeps, never read by a
 * kernel path).  Tests use the difference around a call, e.g. "a frozen projection costs no weight-gradient launch". */
unsigned long long msda_launch_count(void);

/* Test hook: force the kernel family for the CALLING THREAD's subsequent calls (-1 = automatic, default; MSDA_PATH_GENERIC).
 * Thread-local, so no caller can change the kernels under another thread's launch; not meant for production callers. */
void msda_force_path(int path);

#ifdef __cplusplus
}
#endif
#endif /* MSDA_H_ */
