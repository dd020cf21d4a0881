// Host-side plumbing shared by the kernel translation units: the thread-local error
// string behind msda_last_error() and the declarations of the per-family launchers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "msda.h"
#include "msda_common.h"
#include "msda_op_args.h"
#include "msda_set_args.h"

namespace msda {

// Tuning / A-B knobs (MSDA_SPLIT, MSDA_XCD, MSDA_BWD_MODE, MSDA_BWD_WGS, ... tools/README.md) exist only in DIAGNOSTIC
// builds (-DMSDA_TUNING: `make -C uvhand_amd/csrc tuning`, tools/micro/kbench.cpp).  The shipped library reads no
// environment variable and keeps no process-wide state: these helpers then return the default.
#ifdef MSDA_TUNING
#include <cstdlib>
inline const char *tuning_str(const char *name) { const char *v = getenv(name); return (v && *v) ? v : nullptr; }
#else
inline const char *tuning_str(const char *) { return nullptr; }
#endif
inline int tuning_int(const char *name, int dflt) { const char *v = tuning_str(name); return v ? atoi(v) : dflt; }

// Records `msg` for msda_last_error() on this thread and returns `code`.
int set_error(int code, const char *msg);
// Returns MSDA_OK, or records hipGetLastError() (prefixed by `what`) and returns MSDA_ERR_LAUNCH.
int check_launch(const char *what);

// ---- the sampling op: one call = its geometry, tensors and options (msda_op_args.h) ----
// generic family (msda_generic.hip): any D; VT = float, double, or uint16_t (bf16 rows, fp32 everything else)
template <typename VT>
int launch_fwd_generic(const OpGeom &g, const FwdTensors<VT> &t);
template <typename VT>
int launch_bwd_generic(const OpGeom &g, const BwdTensors<VT, op_real_t<VT>> &t, const OpOptions &o);

// ---- D = 32 family (msda_d32.hip): the model's shape -------------------------------------------
// VT = storage of value / out / grad_out: float, or uint16_t (bf16 bits); loc, attn and their gradients are fp32.
// GT = storage of grad_value: VT, or float for bf16 rows (nothing is rounded between the passes of a multi-pass backward,
// and a caller whose value tensor is fp32 needs no conversion of the result).
// table: the buffer a forward can leave for its backward (forward: written, backward: read), or null.
// A backward call's workspace: with forward_table (MSDA_FLAG_FORWARD_TABLE) that table first, the call's scratch behind it.
bool d32_supported(const OpGeom &g);
template <typename VT>
int launch_fwd_d32(const OpGeom &g, const FwdTensors<VT> &t, void *table);
template <typename VT, typename GT>
int launch_bwd_d32(const OpGeom &g, const BwdTensors<VT, GT> &t, const OpOptions &o);
// bytes of that table (0 = the backward's plan reads none)
size_t forward_table_bytes(const OpGeom &g, bool prologue);
inline bool aligned_to(const void *p, size_t bytes) { return ((uintptr_t)p & (bytes - 1)) == 0; }
// The table inside `workspace` (include/msda.h: msda_forward_ws_* fills the start of it, a backward call with
// MSDA_FLAG_FORWARD_TABLE finds it there).  `need` = forward_table_bytes of the geometry: used only where the plan has a
// table and the caller's buffer holds all of it.
inline void *table_of(void *workspace, size_t ws_bytes, size_t need)
{
    return (workspace && aligned_to(workspace, 16) && need > 0 && ws_bytes >= need) ? workspace : nullptr;
}
// ... and the scratch of that backward call: what follows the table, rounded up to 256 bytes (no table: all of the workspace)
inline size_t table_span(size_t table_bytes) { return (table_bytes + 255) & ~(size_t)255; }
struct Scratch { void *p; size_t bytes; };
inline Scratch scratch_behind(void *workspace, size_t ws_bytes, size_t table_bytes)
{
    const size_t span = table_span(table_bytes);
    if (!workspace || ws_bytes <= span) return Scratch{nullptr, 0};
    return Scratch{static_cast<unsigned char *>(workspace) + span, ws_bytes - span};
}
// clears the 'written' stamp of a table buffer that a forward call could not fill (see msda_d32.hip)
int invalidate_forward_table(void *table, const OpGeom &g, hipStream_t stream);
// scratch a D = 32 backward call with these flags can use (0 = none needed); see msda.h
size_t backward_workspace_bytes(const OpGeom &g, unsigned flags);
// number of query chunks ("passes") role B of the D = 32 backward takes for Lq*P sampling points per (b, m, l)
int backward_passes(int Lq, int P);
// text form of the launch plan of a D = 32 geometry (msda_describe_plan); returns the length written.  Of `o` it reads the
// flags and whether there is a workspace (ws_bytes != 0)
int describe_plan(int row_bytes, int gv_bytes, const OpGeom &g, bool prologue, const OpOptions &o, char *buf, int len);

// ---- fused prologue (D = 32 family): softmax over L*P and loc = ref + offset/(W,H) inside the kernels.  Offsets, logits,
// reference points and every gradient are fp32 (grad_value included, for bf16 rows too).  The records' ld_* are validated by
// the ABI layer (>= the dense width, offsets' even).
bool prologue_supported(const OpGeom &g);
template <typename VT>
int launch_fwd_prologue(const OpGeom &g, const FwdTensors<VT> &t, void *table);
template <typename VT>
int launch_bwd_prologue(const OpGeom &g, const BwdTensors<VT, float> &t, const OpOptions &o);

// ---- weight / bias gradient of the bracketing nn.Linear layers (msda_linear.hip) -----------------
size_t linear_wgrad_workspace_bytes(int M, int N, int K);
// row_mask (may be null): one byte per row of dY, non-zero = that row counts as zero
int launch_linear_wgrad(const float *dY, const float *X, const uint8_t *row_mask, int M, int N, int K, float *dW, float *db,
                        float *workspace, hipStream_t stream);
// several fp32 weight gradients: first stages back to back, ONE second stage for all (count <= 4; per-problem arrays)
int launch_linear_wgrad_multi(int count, const void *const *dY, const void *const *X, const int *bf16, const uint8_t *const *row_mask,
                              const int *M, const int *N, const int *K, float *const *dW, float *const *db, float *const *workspace,
                              hipStream_t stream);
// bf16 operands (uint16_t bits), fp32 products / accumulation / results
int launch_linear_wgrad_bf16(const uint16_t *dY, const uint16_t *X, const uint8_t *row_mask, int M, int N, int K, float *dW,
                             float *db, float *workspace, hipStream_t stream);
int launch_zero_masked_rows(float *x, const uint8_t *mask, long long rows, int cols, hipStream_t stream);
// up to four fp32 -> bf16 conversions in one launch (msda_linear.hip)
int launch_cast_bf16_multi(int count, const float *const *src, uint16_t *const *dst, const long long *n, hipStream_t stream);

// ---- forward and input gradient of the same layers (msda_gemm.hip); row_mask (may be null): rows written as zeros ----
int launch_linear_forward(const float *x, const float *w, const float *bias, const uint8_t *row_mask, long long rows,
                          int out_features, int in_features, float *y, hipStream_t stream);
int launch_linear_dgrad(const float *grad_out, const float *w, const uint8_t *row_mask, long long rows, int out_features,
                        int in_features, float *grad_in, hipStream_t stream);

// ---- transformer input assembly (msda_flatten.hip): per-level NCHW <-> the flattened [N, S, C] layout ----
struct FlattenPlan {
    int L;
    float *src[kMaxLevels];          // per level [N, C, H_l, W_l] (device), or null
    float *pos[kMaxLevels];
    int hw[kMaxLevels], start[kMaxLevels], first_block[kMaxLevels];
};
int launch_flatten_levels(const FlattenPlan &plan, int N, int C, int S, const float *level_embed, float *src_flat, float *pos_flat,
                          bool unflatten, hipStream_t stream, float *grad_level_embed = nullptr, float *workspace = nullptr);
size_t unflatten_workspace_bytes(const FlattenPlan &plan, int N, int C);

// ---- residual add + LayerNorm of the layers around the op (msda_layernorm.hip) ---------------------
size_t add_layernorm_workspace_bytes(long long rows, int d);
int launch_add_layernorm_fwd(const float *x, const float *res, const float *gamma, const float *beta, long long rows, int d,
                             float eps, float *y, float *mean, float *rstd, hipStream_t stream);
int launch_add_layernorm_bwd(const float *dy, const float *x, const float *res, const float *gamma, const float *mean,
                             const float *rstd, long long rows, int d, float *ds, float *dgamma, float *dbeta, float *workspace,
                             hipStream_t stream);
int launch_add_layernorm_fwd_bf16res(const float *x, const uint16_t *res, const float *gamma, const float *beta, long long rows,
                                     int d, float eps, float *y, float *mean, float *rstd, hipStream_t stream);
int launch_add_layernorm_bwd_bf16res(const float *dy, const float *x, const uint16_t *res, const float *gamma, const float *mean,
                                     const float *rstd, long long rows, int d, float *ds, uint16_t *ds_bf16, float *dgamma,
                                     float *dbeta, float *workspace, hipStream_t stream);

// ---- FFN of the layers: backward of dropout(relu(h)) in one in-place pass (msda_layernorm.hip) ----
int launch_relu_dropout_bwd(float *grad, const float *act, float scale, long long n, hipStream_t stream);

// ---- two-stage query selection of the transformer (msda_two_stage.hip) ----
constexpr int kSelMaxRows = 8192;  // rows per frame the selection sorts in LDS (64 KB of 64-bit keys)
int launch_two_stage_proposals(const float *memory, const uint8_t *pad, int N, int S, int C, int L, const int *heights,
                               const int *widths, const float *learnedxy, float *proposals, float *memory_out, uint8_t *row_mask,
                               hipStream_t stream);
int launch_two_stage_select(const float *cls, const float *hand, const float *obj, const float *prop, int N, int S, int K, int Q,
                            int hand0, int hand1, int64_t *topk, float *unsig, float *refp, hipStream_t stream);
int launch_pe(const float *r, const float *dim_t, long long M, float *pe, hipStream_t stream);
int launch_pe_linear_relu(const float *r, const float *dim_t, const float *w, const float *bias, long long M, int Nc, float *y,
                          hipStream_t stream);

// ---- the AssemblyHands transformer's refinement and two-stage block (msda_assembly.hip) ----
constexpr int kAssemblySelMaxObj = 14;  // object classes one selection reduces over
int launch_assembly_refine(const float *ref, int width, const float *cls, int K, const float *kp, long long M, float *out,
                           hipStream_t stream);
int launch_assembly_level_proposals(const float *memory, long long mem_frame_stride, const uint8_t *pad, long long pad_frame_stride,
                                    int N, int H, int W, int C, float *proposals, float *memory_out, uint8_t *row_mask,
                                    hipStream_t stream);
int launch_assembly_select(const float *cls, const float *hand, const float *obj, int N, int S, int K, int obj_first, int obj_last,
                           int left, int right, int64_t *indices, float *refp, hipStream_t stream);

// ---- the DINO decoder's query positions and refinement (msda_dino.hip) ----
int launch_dino_sine_embed(const float *ref, int width, const float *valid_xy, int N, long long M, const float *dim_t, float *pe,
                           hipStream_t stream);
int launch_dino_query_pos(const float *ref, int width, const float *valid_xy, int N, long long M, const float *dim_t, const float *w1,
                          const float *b1, const float *w2, const float *b2, float *h, float *y, hipStream_t stream);
int launch_dino_refine_fwd(const float *ref, const float *cls, int K, const float *dkey, const float *dobj, int hand0, int hand1,
                           long long M, float *out, uint8_t *code, hipStream_t stream);
int launch_dino_refine_bwd(const float *gout, const float *out, const uint8_t *code, long long M, float *gkey, float *gobj,
                           hipStream_t stream);

// ---- DINO's two-stage query selection for any number of rows per frame (msda_dino_select.hip); checked arguments ----
constexpr int kDinoSelMaxQueries = 2048;    // queries of a frame (their 64-bit keys are sorted in 16 KB of LDS)
constexpr int kDinoSelMaxRows = 1 << 20;    // rows of a frame (one workgroup reads a frame's keys once per radix digit)
constexpr int kDinoSelMaxFrames = 65535;    // frames (a grid dimension)
size_t dino_select_workspace_bytes(int N, int S);
int launch_dino_select_fwd(const float *cls, const float *memory, const float *proposals, int N, int S, int K, int Q, int C,
                           int hand0, int hand1, int64_t *topk, int32_t *slot, float *tgt, float *prop_sel, uint8_t *code,
                           void *workspace, hipStream_t stream);
int launch_dino_select_bwd(const int32_t *slot, const float *grad_tgt, int N, int S, int Q, int C, float *grad_memory,
                           hipStream_t stream);

// ---- DINO's contrastive-denoising queries and the label embedding's gradient (msda_cdn.hip); checked arguments ----
int launch_cdn_prepare_fwd(const int64_t *labels, const int64_t *offsets, const float *keys, const float *weight, const long long *seed,
                           int B, long long T, int W, int H, long long rows_book, int single_pad, int groups, int num_classes,
                           unsigned thr, float scale, float *out_label, float *out_key, int32_t *noised, float *key_debug,
                           hipStream_t stream);
int launch_cdn_prepare_bwd(const float *grad_label, const int32_t *noised, long long rows, int H, long long rows_book, float *grad_weight,
                           hipStream_t stream);

// ---- the Hungarian matchers: cost block + assignment per (prediction set, frame) (msda_matcher.hip) ----
// per-slot status codes (include/msda.h); the limits, PredSets, SetTargets and MatchView are msda_set_args.h's
constexpr int kMatchInvalid = 1, kMatchInfeasible = 2, kMatchBadLabel = 3, kMatchBadTargets = 4;
int launch_match(const PredSets<const float> &sets, int n_sets, int bs, int Q, int K, int D, const SetTargets &tg, float w_cls,
                 float w_kp, int64_t *out, float *cost_debug, hipStream_t stream);
int launch_lsap(const float *cost, int B, int Q, int T, int64_t *out, hipStream_t stream);

// ---- the set criteria's matched losses over the matcher's device result (msda_criterion.hip) ----
constexpr int kCritArctic = 0, kCritAssembly = 1;
constexpr int kCritTerms = 4;   // loss columns per set (include/msda.h)
constexpr int kCritStats = 4;   // status bits, hand rows, object rows, no valid target (ARCTIC)
constexpr int kCritBadLabel = 1, kCritBadTargets = 2, kCritMaskMismatch = 4, kCritMatchStatus = 8;
struct CritArgs {
    int kind, sets, bs, Q, K, D;
    const int64_t *match;       // the matcher's result buffer
    SetTargets tg;              // is_valid: ARCTIC; NULL for AssemblyHands
    const uint8_t *joint_valid; // AssemblyHands [n_targets, D]
    unsigned long long hand_mask;
    const float *num_boxes;     // device scalar
    float alpha;
};
int launch_criterion_fwd(const CritArgs &a, const PredSets<const float> &p, float *losses, int32_t *stats, hipStream_t stream);
int launch_criterion_bwd(const CritArgs &a, const PredSets<const float> &p, const PredSets<float> &g, const float *grad_losses,
                         const int32_t *stats, hipStream_t stream);

// ---- the DINO criterion's matched and denoising losses (msda_criterion_dino.hip); status bits and columns as above ----
constexpr int kDinoCritChunkRows = 256;      // rows of one frame a forward / backward workgroup covers (include/msda.h)
constexpr int kDinoCritPartialBytes = 64;    // one forward workgroup's partial record in the workspace
struct DinoCritArgs {
    int sets, bs, K, D, match_sets, single_pad, groups;
    const int64_t *match;       // the matcher's result buffer (match_sets sets); NULL when every set is a denoising set
    SetTargets tg;
    unsigned long long hand_mask;
    const float *num_boxes;     // device scalar
    float alpha;
    int Q[kMatchMaxSets];
    int match_set[kMatchMaxSets];    // the set's index in `match`, or -1: a denoising set
    int chunk_base[kMatchMaxSets];   // the set's first chunk; chunk = (set, frame, kDinoCritChunkRows rows of the frame)
    int chunks;                      // of all sets
};
int launch_criterion_dino_fwd(const DinoCritArgs &a, const PredSets<const float> &p, void *workspace, float *losses,
                              int32_t *stats, hipStream_t stream);
int launch_criterion_dino_bwd(const DinoCritArgs &a, const PredSets<const float> &p, const PredSets<float> &g,
                              const float *grad_losses, const int32_t *stats, hipStream_t stream);

// ---- the DeformableDETR prediction heads as grouped GEMMs: fp32 (msda_heads.hip) and bf16 autocast (msda_heads_bf16.hip) ----
// One set of problem tables, one planner (msda_heads.hip) and one workspace layout serve both forms; a table says beside every
// pointer that can be either whether it is bf16, and the fp32 kernels ignore those flags.  Every problem table travels by value
// in the kernel arguments (each struct below stays under 4 KB).
constexpr int kHeadsF32 = 0, kHeadsBf16 = 1;                        // the form of a call / a plan
constexpr int kHeadsMaxLevels = 8, kHeadsMaxMlp = 2, kHeadsShared = 6;
constexpr int kHeadsTile = 64;                                      // output tile edge of every GEMM kernel of both forms
constexpr int kHeadsReduceBlock = 256;                              // heads_reduce_kernel's workgroup: elements per block
constexpr int kHeadsWgradChunk = 2048;                              // rows per weight-gradient partial
constexpr int kHeadsEpiBias = 0, kHeadsEpiRelu = 1, kHeadsEpiArctic = 2, kHeadsEpiAssembly = 3;
constexpr int kHeadsModePlain = 0, kHeadsModeSigmoid = 1, kHeadsModeRelu = 2;
constexpr int kHeadsSrcBf16 = 1, kHeadsSrcVec = 2;                  // HeadsWgradProb::dy_flags
struct HeadsFwdGroup {          // columns [off, off + n) of a problem: one weight [n, C], its bias, its output [L * M, n]
    const float *w, *b;
    void *out;
    int n, off, out_bf16, pad;
};
struct HeadsFwdProb {           // rows [row0, row0 + rows) of the flattened input a [L * M, C]
    const void *a;
    float *sig;                 // keypoint epilogues: the saved sigmoid [L * M, n]
    int row0, rows, n, epi, g0, ng, tile0, a_bf16;
};
constexpr int kHeadsFwdMaxProbs = kHeadsMaxLevels * (1 + kHeadsMaxMlp) + 1;
constexpr int kHeadsFwdMaxGroups = kHeadsFwdMaxProbs + kHeadsShared;
struct HeadsFwdArgs {
    HeadsFwdProb p[kHeadsFwdMaxProbs];
    HeadsFwdGroup g[kHeadsFwdMaxGroups];
    const float *init_ref, *inter_ref;
    int nprob, M, C, R;
};
struct HeadsDgradSeg {          // one reduction segment: dy [L * M, k] o mode (aux: fp32 sigmoids / saved activations) times w [k, C]
    const void *a, *aux;
    const float *w;
    int k, mode, a_bf16, vec;   // vec (bf16 form): k % 8 == 0, 16-byte aligned rows, no sigmoid: 8 elements per load
};
struct HeadsDgradProb {
    void *out;                  // [L * M, C]: a hidden gradient, or fp32 grad_hs
    int row0, rows, s0, ns, tile0, out_bf16;
};
constexpr int kHeadsDgradMaxProbs = kHeadsMaxLevels * kHeadsMaxMlp;
constexpr int kHeadsDgradMaxSegs = kHeadsMaxLevels * (1 + kHeadsMaxMlp + kHeadsShared);
struct HeadsDgradArgs {
    HeadsDgradProb p[kHeadsDgradMaxProbs];
    HeadsDgradSeg s[kHeadsDgradMaxSegs];
    int nprob, C;
};
struct HeadsWgradProb {         // dW [n, C] of one weight over rows [row0, row0 + rows): dy / aux [L * M, n], x [L * M, C]
    const void *dy, *aux, *x;
    long long part;             // float offset of its partials in the workspace: [chunks][n][C], then [chunks][n]
    int row0, rows, n, mode, chunks, tile0, dy_flags, x_bf16;      // dy_flags: kHeadsSrcBf16 | kHeadsSrcVec (as HeadsDgradSeg::vec)
};
constexpr int kHeadsWgradMaxProbs = kHeadsMaxLevels * (1 + 3 * kHeadsMaxMlp) + kHeadsShared;
struct HeadsWgradArgs {
    HeadsWgradProb p[kHeadsWgradMaxProbs];
    float *ws;
    int nprob, C;
};
struct HeadsReduceProb {
    long long part;
    float *dw, *db;
    int n, chunks, tile0, pad;  // tile0: its first workgroup
};
struct HeadsReduceArgs {
    HeadsReduceProb p[kHeadsWgradMaxProbs];
    const float *ws;
    int nprob, C;
};
static_assert(sizeof(HeadsFwdArgs) <= 4000 && sizeof(HeadsDgradArgs) <= 4000 && sizeof(HeadsWgradArgs) <= 4000
              && sizeof(HeadsReduceArgs) <= 4000, "kernel argument tables");

// One call's operands as the C entries receive them (include/msda.h, msda_heads_*), in either form.  hs, the parameters, the
// references, sig and every parameter gradient are fp32 in both; the operands behind void pointers are fp32 in the fp32 form
// and carry the dtypes of torch's bf16 autocast in the bf16 form: hidden, the shared outputs and their gradients bf16; logits /
// keypoints and their gradients fp32 (ARCTIC) or bf16 (AssemblyHands).
struct HeadsCall {
    int form, kind, L, n_mlp, R, C, K;
    long long M;
    unsigned flags;
    const float *hs, *init_ref, *inter_ref;
    const float *const *cls_w, *const *cls_b, *const *mlp_w, *const *mlp_b, *const *shared_w, *const *shared_b;
    void *logits, *const *kp_out, *const *shared_out, *hidden;
    float *sig;
    const void *grad_logits, *const *grad_kp, *const *grad_shared;
    float *grad_hs, *const *grad_cls_w, *const *grad_cls_b, *const *grad_mlp_w, *const *grad_mlp_b, *const *grad_shared_w,
        *const *grad_shared_b;
    void *ws;
    unsigned long long ws_bytes;
};
struct HeadsFwdPlan {
    HeadsFwdArgs a[3];
    int tiles[3], form;
};
struct HeadsBwdPlan {
    HeadsDgradArgs d[3];
    int dtiles[3];
    HeadsWgradArgs w;
    int wtiles;
    HeadsReduceArgs r;
    int rblocks, form;
};
// The planner (msda_heads.hip): plan_* checks the call and builds the problem tables without launching anything, run_* launches
// the plan's tables on its form's kernels.
bool heads_supported(int form, int C);
unsigned long long heads_workspace_bytes(int form, int kind, int L, long long M, int C, int K, int n_mlp, unsigned flags);
int heads_plan_forward(const HeadsCall &c, HeadsFwdPlan &plan);
int heads_plan_backward(const HeadsCall &c, HeadsBwdPlan &plan);
int heads_run_forward(const HeadsFwdPlan &plan, hipStream_t stream);
int heads_run_backward(const HeadsBwdPlan &plan, hipStream_t stream);
// the reference gradient of the ARCTIC keypoint epilogue (msda_heads_ref_backward_f32): the flat element space [L * M * R]
struct HeadsRefBwdArgs {
    const float *init_ref, *inter_ref, *sig, *grad_kp[kHeadsMaxMlp];
    float *grad_init_ref, *grad_inter_ref;
    long long MR, LMR, e0, groups;          // M * R, L * M * R, the first element written, groups of the access width
};
struct HeadsRefBwdPlan {
    HeadsRefBwdArgs a;
    int blocks, width;                      // zero blocks: no output asked for, no launch
};
int heads_plan_ref_backward(int L, long long M, int n_mlp, int R, const float *init_ref, const float *inter_ref, const float *sig,
                            const float *const *grad_kp, float *grad_init_ref, float *grad_inter_ref, HeadsRefBwdPlan &plan);
int heads_run_ref_backward(const HeadsRefBwdPlan &plan, hipStream_t stream);
// the bf16 form's kernels (msda_heads_bf16.hip); zero tiles: no launch
int launch_heads_forward_bf16(const HeadsFwdArgs &a, int tiles, hipStream_t stream);
int launch_heads_dgrad_bf16(const HeadsDgradArgs &a, int tiles, hipStream_t stream);
int launch_heads_wgrad_bf16(const HeadsWgradArgs &a, int tiles, hipStream_t stream);
// one grid of `groups` workgroups of 256 threads, none when groups == 0
template <class Args>
int heads_launch(void (*kernel)(Args), const char *name, const Args &a, int groups, hipStream_t stream)
{
    if (groups == 0) return MSDA_OK;
    hipLaunchKernelGGL(kernel, dim3((unsigned)groups), dim3(256), 0, stream, a);
    return check_launch(name);
}

// ---- the layers' FFN under bf16 autocast (msda_ffn_bf16.hip; C entries msda_ffn_*_bf16): the checks return MSDA_OK or an
// argument error and launch nothing; the launchers take checked arguments ----
bool ffn_bf16_supported(int C, int F);
size_t ffn_bf16_workspace_bytes(long long M, int C, int F);
int ffn_check_forward_bf16(long long M, int C, int F, const void *x, int x_is_bf16, const float *w1, const float *b1, const float *w2,
                           const float *b2, double p, const long long *seed, const uint16_t *xb, const uint16_t *a, const uint16_t *y);
int launch_ffn_forward_bf16(long long M, int C, int F, const void *x, int x_is_bf16, const float *w1, const float *b1, const float *w2,
                            const float *b2, double p, const long long *seed, uint16_t *xb, uint16_t *a, uint16_t *y,
                            hipStream_t stream);
int ffn_check_backward_bf16(long long M, int C, int F, const uint16_t *grad_out, const uint16_t *xb, const uint16_t *a, const float *w1,
                            const float *w2, double p, const void *grad_x, const float *grad_w1, const float *grad_b1,
                            const float *grad_w2, const float *grad_b2, const void *workspace, unsigned long long workspace_bytes);
int launch_ffn_backward_bf16(long long M, int C, int F, const uint16_t *grad_out, const uint16_t *xb, const uint16_t *a, const float *w1,
                             const float *w2, double p, void *grad_x, int grad_x_is_bf16, float *grad_w1, float *grad_b1,
                             float *grad_w2, float *grad_b2, void *workspace, hipStream_t stream);

// ---- Swin window attention, head_dim 32, windows up to 12 x 12 (msda_swin.hip; C entries msda_swin_attn_*) ----
bool swin_supported(int B, int H, int W, int C, int nH, int ws, int shift);
unsigned long long swin_workspace_bytes(int B, int H, int W, int C, int nH, int ws, int shift, int which);
int swin_forward(int B, int H, int W, int C, int nH, int ws, int shift, const float *qkv, const float *bias, const float *table,
                 float *out, float *lse, unsigned long long lse_bytes, hipStream_t stream);
int swin_backward(int B, int H, int W, int C, int nH, int ws, int shift, const float *qkv, const float *bias, const float *table,
                  const float *out, const float *lse, unsigned long long lse_bytes, const float *grad_out, float *grad_qkv,
                  float *grad_table, float *grad_bias, void *workspace, unsigned long long workspace_bytes, hipStream_t stream);
// bf16 qkv / out / grad_out / grad_qkv (bf16 MFMA, fp32 softmax); bias, table, lse, grad_table, grad_bias and the partials fp32
int swin_forward_bf16(int B, int H, int W, int C, int nH, int ws, int shift, const uint16_t *qkv, const float *bias,
                      const float *table, uint16_t *out, float *lse, unsigned long long lse_bytes, hipStream_t stream);
int swin_backward_bf16(int B, int H, int W, int C, int nH, int ws, int shift, const uint16_t *qkv, const float *bias,
                       const float *table, const uint16_t *out, const float *lse, unsigned long long lse_bytes,
                       const uint16_t *grad_out, uint16_t *grad_qkv, float *grad_table, float *grad_bias, void *workspace,
                       unsigned long long workspace_bytes, hipStream_t stream);

// ---- the Swin blocks' residual / drop-path / LayerNorm glue and PatchMerging's gather + norm (msda_swin_glue.hip; C entries
// msda_swin_glue_*).  bf16: a, keep, z and their gradients are bf16 bits (uint16_t), else float.  sbf16: the residual stream (x,
// y and their gradients) is bf16 bits, else float; a bf16 stream has a bf16 branch, and fp32 z for norm alone.  Statistics fp32.
bool swin_glue_supported(int C);
unsigned long long swin_glue_workspace_bytes(long long rows, int C);
int swin_glue_norm_forward(bool sbf16, bool bf16, const void *x, const float *gamma, const float *beta, long long rows, int C,
                           float eps, void *z, float *mean, float *rstd, hipStream_t stream);
int swin_glue_norm_backward(bool sbf16, bool bf16, const void *grad_z, const void *x, const float *gamma, const float *mean,
                            const float *rstd, long long rows, int C, void *grad_x, float *grad_gamma, float *grad_beta,
                            void *workspace, unsigned long long workspace_bytes, hipStream_t stream);
int swin_glue_add_norm_forward(bool sbf16, bool bf16, const void *x, const void *a, const void *keep, long long rows,
                               long long rows_per_sample, int C, const float *gamma, const float *beta, float eps, void *y,
                               void *z, float *mean, float *rstd, hipStream_t stream);
int swin_glue_add_norm_backward(bool sbf16, bool bf16, const void *grad_y, const void *grad_z, const void *y, const void *keep,
                                const float *gamma, const float *mean, const float *rstd, long long rows,
                                long long rows_per_sample, int C, void *grad_x, void *grad_a, float *grad_gamma,
                                float *grad_beta, void *workspace, unsigned long long workspace_bytes, hipStream_t stream);
int swin_glue_add_forward(bool sbf16, bool bf16, const void *x, const void *a, const void *keep, long long rows,
                          long long rows_per_sample, int C, void *y, hipStream_t stream);
int swin_glue_add_backward(bool sbf16, bool bf16, const void *grad_y, const void *keep, long long rows,
                           long long rows_per_sample, int C, void *grad_a, hipStream_t stream);
int swin_glue_merge_norm_forward(bool sbf16, bool bf16, const void *x, int B, int H, int W, int C, const float *gamma,
                                 const float *beta, float eps, void *z, float *mean, float *rstd, hipStream_t stream);
int swin_glue_merge_norm_backward(bool sbf16, bool bf16, const void *grad_z, const void *x, const float *gamma,
                                  const float *mean, const float *rstd, int B, int H, int W, int C, void *grad_x,
                                  float *grad_gamma, float *grad_beta, void *workspace, unsigned long long workspace_bytes,
                                  hipStream_t stream);

// ---- the input-projection neck: bias + GroupNorm + feature mask of every level (msda_neck.hip; C entries msda_neck_*) ----
// Both level tables travel by value in the kernel arguments, as FlattenPlan does.
constexpr int kNeckMaxLevels = 8;
struct NeckFwdPlan {
    int L;
    const float *y[kNeckMaxLevels], *bias[kNeckMaxLevels], *gamma[kNeckMaxLevels], *beta[kNeckMaxLevels], *u[kNeckMaxLevels];
    float *out[kNeckMaxLevels], *mean[kNeckMaxLevels], *rstd[kNeckMaxLevels];
    unsigned char *mask[kNeckMaxLevels];
    int hw[kNeckMaxLevels], vec[kNeckMaxLevels], first_block[kNeckMaxLevels];
};
struct NeckBwdPlan {
    int L;
    const float *grad_out[kNeckMaxLevels], *y[kNeckMaxLevels], *bias[kNeckMaxLevels], *gamma[kNeckMaxLevels];
    const float *mean[kNeckMaxLevels], *rstd[kNeckMaxLevels];
    const unsigned char *mask[kNeckMaxLevels];
    float *grad_y[kNeckMaxLevels], *grad_gamma[kNeckMaxLevels], *grad_beta[kNeckMaxLevels], *grad_bias[kNeckMaxLevels];
    float *partial[kNeckMaxLevels];      // [3][N][C] per level
    int hw[kNeckMaxLevels], vec[kNeckMaxLevels], first_block[kNeckMaxLevels];
};
static_assert(sizeof(NeckFwdPlan) <= 2000 && sizeof(NeckBwdPlan) <= 2000, "kernel argument tables");
bool neck_supported(int L, int N, int C, int groups, const int *heights, const int *widths);
size_t neck_workspace_bytes(int L, int N, int C);
int launch_neck_forward(const NeckFwdPlan &plan, int N, int C, int groups, float eps, hipStream_t stream);
int launch_neck_backward(const NeckBwdPlan &plan, int N, int C, int groups, hipStream_t stream);

// ---- the tail of the step: gradient norm, clip and AdamW as multi-tensor launches (msda_optim.hip; C entries msda_optim_*,
// msda_grad_*, msda_adamw_step_f32).  Every table is a DEVICE array the caller owns, one entry per tensor (chunk_start: n + 1);
// the per-group hyperparameters are host arrays and travel by value in the kernel arguments.  Every check is the launcher's.
constexpr int kOptimChunk = 8192;     // elements of a chunk: one workgroup
constexpr int kOptimMaxGroups = 8;
struct OptimTables {
    int n;
    long long n_chunks;
    float *const *p;
    const float *const *g;
    float *const *exp_avg, *const *exp_avg_sq;
    const long long *numel, *chunk_start;
    const int *group;
    const long long *step_offset;
};
bool optim_supported(long long n_tensors, int n_groups);
long long optim_chunks(int n, const long long *numel, long long *chunk_start);      // host arrays; -1: argument error
int launch_grad_sumsq(int n, long long n_chunks, const float *const *g, const long long *numel, const long long *chunk_start,
                      float *partials, hipStream_t stream);
int launch_grad_norm_finish(long long n_chunks, const float *partials, float max_norm, float *out, hipStream_t stream);
int launch_grad_scale(int n, long long n_chunks, float *const *g, const long long *numel, const long long *chunk_start,
                      const float *coef, hipStream_t stream);
int launch_adamw_step(const OptimTables &t, int n_groups, const double *lr, const double *weight_decay, const double *beta1,
                      const double *beta2, const double *eps, long long global_step, const float *coef, hipStream_t stream);
// the device-state forms (msda_optim_advance_f32, msda_grad_norm_finish_dev_f32, msda_adamw_step_dev_f32): step is a DEVICE table
// of pointers to 0-d fp32 device steps, hyper a DEVICE table [n_groups][5] of lr, weight_decay, beta1, beta2, eps; t.step_offset
// is not read
int launch_optim_advance(int n, float *const *step, hipStream_t stream);
int launch_grad_norm_finish_dev(long long n_chunks, const float *partials, float max_norm, float *out, int n, float *const *step,
                                int skip_nonfinite, int *status, hipStream_t stream);
int launch_adamw_step_dev(const OptimTables &t, const float *const *step, int n_groups, const double *hyper, const float *coef,
                          const int *skip, hipStream_t stream);

}  // namespace msda
