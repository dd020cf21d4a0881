// C ABI of libmsda_hip.so (declared in include/msda.h): argument validation, kernel-family
// selection, error reporting.  No torch types, no allocation, no device synchronisation.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <string>

#include <atomic>

#include "msda_launch.h"

namespace msda {

static thread_local char g_err[512] = "";
static thread_local int g_force_path = -1;          // msda_force_path(): test hook, this thread's calls only

int set_error(int code, const char *msg)
{
    std::snprintf(g_err, sizeof(g_err), "%s", msg ? msg : "unknown error");
    return code;
}

// Start of every entry point that enqueues work: forget this thread's previous message and any sticky
// error an unrelated earlier HIP call left behind, so that check_launch() reports THIS call's launch only.
static void begin_call()
{
    g_err[0] = 0;
    (void)hipGetLastError();
}

// Launches enqueued by this process through the library (every launcher ends in check_launch, once per kernel it queued or
// per pair of dependent kernels): a diagnostic for tests ("a frozen projection costs no weight-gradient launch"), relaxed atomic.
static std::atomic<unsigned long long> g_launch_checks{0};
unsigned long long launch_checks() { return g_launch_checks.load(std::memory_order_relaxed); }

int check_launch(const char *what)
{
    g_launch_checks.fetch_add(1, std::memory_order_relaxed);
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return MSDA_OK;
    char buf[400];
    std::snprintf(buf, sizeof(buf), "%s: %s", what, hipGetErrorString(e));
    return set_error(MSDA_ERR_LAUNCH, buf);
}

// ---- the sampling op: every entry fills the records of msda_op_args.h and calls one of the four bodies below ----
static int check_args(const OpGeom &g, std::initializer_list<const void *> ptrs)
{
    if (g.N < 0 || g.S < 0 || g.M <= 0 || g.D <= 0 || g.L <= 0 || g.Lq < 0 || g.P <= 0)
        return set_error(MSDA_ERR_ARGUMENT, "msda: sizes must be positive (N, S, Lq may be 0)");
    if (g.N == 0 || g.Lq == 0 || g.S == 0) return MSDA_OK;        // nothing to read
    for (const void *p : ptrs)
        if (p == nullptr) return set_error(MSDA_ERR_ARGUMENT, "msda: null device pointer");
    return MSDA_OK;
}

// Row strides of the fused-prologue tensors: 0 selects the dense layout; otherwise at least the dense
// width, and for the (x, y) pairs an even stride on an 8-byte aligned base (the kernels move float2).
static int check_row_strides(const char *who, const OpGeom &g, const void *offsets, long long *ld_offsets, long long *ld_logits)
{
    const long long dense = (long long)g.M * g.L * g.P;
    if (*ld_offsets == 0) *ld_offsets = 2 * dense;
    if (*ld_logits == 0) *ld_logits = dense;
    char buf[200];
    if (*ld_offsets < 2 * dense || *ld_logits < dense || (*ld_offsets & 1) || ((uintptr_t)offsets & 7) ||
        *ld_offsets - 2 * dense > 0x7fffffffLL || *ld_logits - dense > 0x7fffffffLL) {
        std::snprintf(buf, sizeof(buf), "%s: row strides (%lld, %lld) must be >= (%lld, %lld), the first even on an "
                      "8-byte aligned base", who, *ld_offsets, *ld_logits, 2 * dense, dense);
        return set_error(MSDA_ERR_ARGUMENT, buf);
    }
    return MSDA_OK;
}

// The D = 32 kernels move rows as 16-byte (fp32) / 8-byte (bf16) vectors — grad_value by ITS storage — and locations as
// (x, y) pairs.  Tensors straight from an allocator always qualify; a contiguous VIEW at an odd element offset does not —
// fp32 / bf16 op calls then take the generic kernels (element-wise accesses); the prologue and wgrad entries refuse.
template <typename VT, typename GT = VT>
static bool rows_aligned(std::initializer_list<const void *> rows, const void *grad_value, std::initializer_list<const void *> xy)
{
    for (const void *p : rows) if (!aligned_to(p, sizeof(VT) * 4)) return false;
    for (const void *p : xy) if (!aligned_to(p, 8)) return false;
    return aligned_to(grad_value, sizeof(GT) * 4);
}

static int refuse_unaligned(const char *who)
{
    char buf[200];
    std::snprintf(buf, sizeof(buf), "%s: row tensors must be 16-byte (fp32) / 8-byte (bf16) aligned and (x, y) tensors "
                  "8-byte aligned (a contiguous view at an odd element offset is not)", who);
    return set_error(MSDA_ERR_ARGUMENT, buf);
}

static bool use_d32(const OpGeom &g) { return g_force_path != MSDA_PATH_GENERIC && d32_supported(g); }
static bool prologue_ok(const OpGeom &g) { return g.nonempty() && g_force_path != MSDA_PATH_GENERIC && prologue_supported(g); }
// bytes of the table a forward of this geometry leaves for its backward (msda_forward_workspace_bytes)
static size_t table_need(const OpGeom &g, bool prologue)
{
    return (g.nonempty() && g_force_path != MSDA_PATH_GENERIC) ? forward_table_bytes(g, prologue) : 0;
}

// An empty problem's outputs: the spans that have bytes are zero-filled on the stream.
struct ZeroSpan { void *p; size_t bytes; };
static int zero_fill(hipStream_t stream, std::initializer_list<ZeroSpan> spans)
{
    for (const ZeroSpan &s : spans) {
        if (s.bytes == 0) continue;
        const hipError_t e = hipMemsetAsync(s.p, 0, s.bytes, stream);
        if (e != hipSuccess) return set_error(MSDA_ERR_LAUNCH, hipGetErrorString(e));
    }
    return MSDA_OK;
}

// The four bodies.  fp64 rows never take the D = 32 family; fp32 / bf16 rows take it where the geometry qualifies (use_d32)
// and every tensor is aligned for its vector accesses, else the generic kernels.
template <typename VT>
static int forward_body(const OpGeom &g, const FwdTensors<VT> &t, const OpOptions &o)
{
    if (int rc = check_args(g, {t.value, t.shapes, t.level_start, t.loc, t.attn, t.out})) return rc;
    begin_call();
    if (g.N == 0 || g.Lq == 0) return MSDA_OK;                      // empty output
    if (g.S == 0) return zero_fill(t.stream, {{t.out, sizeof(VT) * (size_t)g.items() * g.D}});   // no pixels: every tap is outside
    void *table = table_of(o.workspace, o.ws_bytes, table_need(g, false));
    if constexpr (sizeof(VT) != 8) {
        if (use_d32(g) && rows_aligned<VT>({t.value, t.out}, nullptr, {t.loc})) return launch_fwd_d32<VT>(g, t, table);
    }
    // (the generic kernels write no table: a buffer the caller handed over gets its stamp cleared)
    if (table) if (int rc = invalidate_forward_table(table, g, t.stream)) return rc;
    return launch_fwd_generic<VT>(g, t);
}

template <typename VT, typename GT>
static int backward_body(const OpGeom &g, const BwdTensors<VT, GT> &t, const OpOptions &o)
{
    if (int rc = check_args(g, {t.grad_out, t.value, t.shapes, t.level_start, t.loc, t.attn, t.grad_value, t.grad_loc, t.grad_attn}))
        return rc;
    begin_call();
    if (g.N == 0) return MSDA_OK;
    if (g.Lq == 0 || g.S == 0) {                                    // no contributions at all
        const size_t points = (size_t)g.items() * g.L * g.P, real = sizeof(op_real_t<VT>);
        return zero_fill(t.stream, {{t.grad_value, sizeof(GT) * (size_t)g.N * g.S * g.M * g.D}, {t.grad_loc, real * points * 2},
                                    {t.grad_attn, real * points}});
    }
    if constexpr (sizeof(VT) != 8) {
        if (use_d32(g) && rows_aligned<VT, GT>({t.grad_out, t.value}, t.grad_value, {t.loc, t.grad_loc}))
            return launch_bwd_d32<VT, GT>(g, t, o);
    }
    if constexpr (sizeof(GT) == 2)
        return set_error(MSDA_ERR_ARGUMENT, "msda_backward_bf16: bf16 grad_value needs the D=32 kernel family (D == 32, "
                                            "L <= 16, L*P <= 32, 8-byte aligned rows); msda_backward_bf16_gv32 serves "
                                            "every other shape");
    else                                                            // element-wise accesses: any D, any element offset
        return launch_bwd_generic<VT>(g, t, o);
}

static int refuse_geometry(const char *who)
{
    char buf[120];
    std::snprintf(buf, sizeof(buf), "%s: geometry not supported (msda_prologue_supported)", who);
    return set_error(MSDA_ERR_ARGUMENT, buf);
}

// who: the entry's name in messages (the _ws_ forms report under the plain names).  t by value: the row strides are resolved here.
template <typename VT>
static int forward_prologue_body(const char *who, const OpGeom &g, FwdTensors<VT> t, const OpOptions &o)
{
    if (int rc = check_args(g, {t.value, t.shapes, t.level_start, t.ref, t.loc, t.attn, t.out, t.loc_out, t.attn_out})) return rc;
    if (!prologue_ok(g)) return refuse_geometry(who);
    if (int rc = check_row_strides(who, g, t.loc, &t.ld_offsets, &t.ld_logits)) return rc;
    if (!rows_aligned<VT>({t.value, t.out}, nullptr, {t.ref, t.loc_out})) return refuse_unaligned(who);
    begin_call();
    return launch_fwd_prologue<VT>(g, t, table_of(o.workspace, o.ws_bytes, table_need(g, true)));
}

template <typename VT>
static int backward_prologue_body(const char *who, const OpGeom &g, BwdTensors<VT, float> t, const OpOptions &o)
{
    if (int rc = check_args(g, {t.grad_out, t.value, t.shapes, t.level_start, t.loc, t.attn, t.grad_value, t.grad_loc, t.grad_attn,
                                t.grad_ref})) return rc;
    if (!prologue_ok(g)) return refuse_geometry(who);
    if (int rc = check_row_strides(who, g, t.grad_loc, &t.ld_grad_offsets, &t.ld_grad_logits)) return rc;
    if (!rows_aligned<VT, float>({t.grad_out, t.value}, t.grad_value, {t.loc, t.grad_ref})) return refuse_unaligned(who);
    begin_call();
    return launch_bwd_prologue<VT>(g, t, o);
}

}  // namespace msda

extern "C" {

int msda_forward_f32(const float *value, const int64_t *spatial_shapes, const int64_t *level_start,
                     const float *sampling_loc, const float *attn_weight, int N, int S, int M, int D,
                     int L, int Lq, int P, float *out, msda_stream_t stream)
{
    return msda::forward_body<float>({N, S, M, D, L, Lq, P}, {value, spatial_shapes, level_start, sampling_loc, attn_weight, out,
                                                              (hipStream_t)stream}, {});
}

int msda_backward_f32(const float *grad_out, const float *value, const int64_t *spatial_shapes,
                      const int64_t *level_start, const float *sampling_loc, const float *attn_weight,
                      int N, int S, int M, int D, int L, int Lq, int P, float *grad_value,
                      float *grad_sampling_loc, float *grad_attn_weight, msda_stream_t stream)
{
    return msda_backward_ws_f32(grad_out, value, spatial_shapes, level_start, sampling_loc, attn_weight, N, S, M, D, L, Lq, P,
                                grad_value, grad_sampling_loc, grad_attn_weight, nullptr, 0, 0, stream);
}

int msda_forward_f64(const double *value, const int64_t *spatial_shapes, const int64_t *level_start,
                     const double *sampling_loc, const double *attn_weight, int N, int S, int M, int D,
                     int L, int Lq, int P, double *out, msda_stream_t stream)
{
    return msda::forward_body<double>({N, S, M, D, L, Lq, P}, {value, spatial_shapes, level_start, sampling_loc, attn_weight, out,
                                                               (hipStream_t)stream}, {});
}

int msda_backward_f64(const double *grad_out, const double *value, const int64_t *spatial_shapes,
                      const int64_t *level_start, const double *sampling_loc,
                      const double *attn_weight, int N, int S, int M, int D, int L, int Lq, int P,
                      double *grad_value, double *grad_sampling_loc, double *grad_attn_weight,
                      msda_stream_t stream)
{
    return msda_backward_ws_f64(grad_out, value, spatial_shapes, level_start, sampling_loc, attn_weight, N, S, M, D, L, Lq, P,
                                grad_value, grad_sampling_loc, grad_attn_weight, nullptr, 0, 0, stream);
}

int msda_forward_bf16(const uint16_t *value, const int64_t *spatial_shapes, const int64_t *level_start,
                      const float *sampling_loc, const float *attn_weight, int N, int S, int M, int D, int L,
                      int Lq, int P, uint16_t *out, msda_stream_t stream)
{
    return msda::forward_body<uint16_t>({N, S, M, D, L, Lq, P}, {value, spatial_shapes, level_start, sampling_loc, attn_weight, out,
                                                                 (hipStream_t)stream}, {});
}

// ---- forward that leaves the point table for the backward of the same autograd node (include/msda.h) ----
unsigned long long msda_forward_workspace_bytes(int N, int S, int M, int D, int L, int Lq, int P, unsigned flags)
{
    return (unsigned long long)msda::table_need({N, S, M, D, L, Lq, P}, (flags & MSDA_FLAG_PROLOGUE) != 0);
}

int msda_forward_ws_f32(const float *value, const int64_t *spatial_shapes, const int64_t *level_start, const float *sampling_loc,
                        const float *attn_weight, int N, int S, int M, int D, int L, int Lq, int P, float *out, void *workspace,
                        unsigned long long workspace_bytes, msda_stream_t stream)
{
    return msda::forward_body<float>({N, S, M, D, L, Lq, P}, {value, spatial_shapes, level_start, sampling_loc, attn_weight, out,
                                                              (hipStream_t)stream}, {workspace, workspace_bytes});
}

int msda_forward_ws_bf16(const uint16_t *value, const int64_t *spatial_shapes, const int64_t *level_start, const float *sampling_loc,
                         const float *attn_weight, int N, int S, int M, int D, int L, int Lq, int P, uint16_t *out, void *workspace,
                         unsigned long long workspace_bytes, msda_stream_t stream)
{
    return msda::forward_body<uint16_t>({N, S, M, D, L, Lq, P}, {value, spatial_shapes, level_start, sampling_loc, attn_weight, out,
                                                                 (hipStream_t)stream}, {workspace, workspace_bytes});
}

int msda_backward_bf16(const uint16_t *grad_out, const uint16_t *value, const int64_t *spatial_shapes,
                       const int64_t *level_start, const float *sampling_loc, const float *attn_weight, int N,
                       int S, int M, int D, int L, int Lq, int P, uint16_t *grad_value, float *grad_sampling_loc,
                       float *grad_attn_weight, msda_stream_t stream)
{
    return msda_backward_ws_bf16(grad_out, value, spatial_shapes, level_start, sampling_loc, attn_weight, N, S, M, D, L, Lq, P,
                                 grad_value, grad_sampling_loc, grad_attn_weight, nullptr, 0, 0, stream);
}

int msda_backward_bf16_gv32(const uint16_t *grad_out, const uint16_t *value, const int64_t *spatial_shapes,
                            const int64_t *level_start, const float *sampling_loc, const float *attn_weight, int N,
                            int S, int M, int D, int L, int Lq, int P, float *grad_value, float *grad_sampling_loc,
                            float *grad_attn_weight, msda_stream_t stream)
{
    return msda_backward_ws_bf16_gv32(grad_out, value, spatial_shapes, level_start, sampling_loc, attn_weight, N, S, M, D, L, Lq, P,
                                      grad_value, grad_sampling_loc, grad_attn_weight, nullptr, 0, 0, stream);
}

int msda_backward_passes(int Lq, int P) { return (Lq > 0 && P > 0) ? msda::backward_passes(Lq, P) : 0; }

unsigned long long msda_backward_workspace_bytes(int N, int S, int M, int D, int L, int Lq, int P, unsigned flags)
{
    const msda::OpGeom g{N, S, M, D, L, Lq, P};
    if (!g.nonempty() || msda::g_force_path == MSDA_PATH_GENERIC) return 0;
    // with MSDA_FLAG_FORWARD_TABLE: the forward's table (rounded up to 256 bytes) first, the call's scratch behind it
    const size_t table = (flags & MSDA_FLAG_FORWARD_TABLE) ? msda::forward_table_bytes(g, (flags & MSDA_FLAG_PROLOGUE) != 0) : 0;
    const size_t scratch = msda::backward_workspace_bytes(g, flags);
    if (table == 0) return (unsigned long long)scratch;
    return (unsigned long long)(scratch ? msda::table_span(table) + scratch : table);
}

int msda_deterministic_supported(int elem_bytes, int N, int S, int M, int D, int L, int Lq, int P)
{
    const msda::OpGeom g{N, S, M, D, L, Lq, P};
    if (!g.nonempty()) return 1;                                                                      // (nothing to order)
    if (elem_bytes != 8 && msda::use_d32(g)) return 1;
    return (double)N * (double)S * (double)M * (double)Lq * (double)P <= 68719476736.0 ? 1 : 0;      // msda_generic.hip: 2^36 point tests
}

int msda_backward_ws_f32(const float *grad_out, const float *value, const int64_t *spatial_shapes,
                         const int64_t *level_start, const float *sampling_loc, const float *attn_weight,
                         int N, int S, int M, int D, int L, int Lq, int P, float *grad_value,
                         float *grad_sampling_loc, float *grad_attn_weight, void *workspace,
                         unsigned long long workspace_bytes, unsigned flags, msda_stream_t stream)
{
    return msda::backward_body<float, float>({N, S, M, D, L, Lq, P},
                                             {grad_out, value, spatial_shapes, level_start, sampling_loc, attn_weight, grad_value,
                                              grad_sampling_loc, grad_attn_weight, (hipStream_t)stream},
                                             {workspace, workspace_bytes, flags});
}

int msda_backward_ws_f64(const double *grad_out, const double *value, const int64_t *spatial_shapes,
                         const int64_t *level_start, const double *sampling_loc, const double *attn_weight,
                         int N, int S, int M, int D, int L, int Lq, int P, double *grad_value,
                         double *grad_sampling_loc, double *grad_attn_weight, void *workspace,
                         unsigned long long workspace_bytes, unsigned flags, msda_stream_t stream)
{
    return msda::backward_body<double, double>({N, S, M, D, L, Lq, P},
                                               {grad_out, value, spatial_shapes, level_start, sampling_loc, attn_weight, grad_value,
                                                grad_sampling_loc, grad_attn_weight, (hipStream_t)stream},
                                               {workspace, workspace_bytes, flags});
}

int msda_backward_ws_bf16(const uint16_t *grad_out, const uint16_t *value, const int64_t *spatial_shapes,
                          const int64_t *level_start, const float *sampling_loc, const float *attn_weight, int N,
                          int S, int M, int D, int L, int Lq, int P, uint16_t *grad_value, float *grad_sampling_loc,
                          float *grad_attn_weight, void *workspace, unsigned long long workspace_bytes,
                          unsigned flags, msda_stream_t stream)
{
    return msda::backward_body<uint16_t, uint16_t>({N, S, M, D, L, Lq, P},
                                                   {grad_out, value, spatial_shapes, level_start, sampling_loc, attn_weight,
                                                    grad_value, grad_sampling_loc, grad_attn_weight, (hipStream_t)stream},
                                                   {workspace, workspace_bytes, flags});
}

int msda_backward_ws_bf16_gv32(const uint16_t *grad_out, const uint16_t *value, const int64_t *spatial_shapes,
                               const int64_t *level_start, const float *sampling_loc, const float *attn_weight, int N,
                               int S, int M, int D, int L, int Lq, int P, float *grad_value, float *grad_sampling_loc,
                               float *grad_attn_weight, void *workspace, unsigned long long workspace_bytes,
                               unsigned flags, msda_stream_t stream)
{
    return msda::backward_body<uint16_t, float>({N, S, M, D, L, Lq, P},
                                                {grad_out, value, spatial_shapes, level_start, sampling_loc, attn_weight,
                                                 grad_value, grad_sampling_loc, grad_attn_weight, (hipStream_t)stream},
                                                {workspace, workspace_bytes, flags});
}

int msda_prologue_supported(int N, int S, int M, int D, int L, int Lq, int P) { return msda::prologue_ok({N, S, M, D, L, Lq, P}) ? 1 : 0; }

int msda_forward_prologue_f32(const float *value, const int64_t *spatial_shapes, const int64_t *level_start,
                              const float *reference_points, const float *sampling_offsets, const float *attn_logits,
                              int N, int S, int M, int D, int L, int Lq, int P, long long ld_offsets, long long ld_logits,
                              float *out, float *sampling_loc_out, float *attn_weight_out, msda_stream_t stream)
{
    return msda_forward_prologue_ws_f32(value, spatial_shapes, level_start, reference_points, sampling_offsets, attn_logits, N, S, M,
                                        D, L, Lq, P, ld_offsets, ld_logits, out, sampling_loc_out, attn_weight_out, nullptr, 0, stream);
}

int msda_forward_prologue_ws_f32(const float *value, const int64_t *spatial_shapes, const int64_t *level_start,
                                 const float *reference_points, const float *sampling_offsets, const float *attn_logits,
                                 int N, int S, int M, int D, int L, int Lq, int P, long long ld_offsets, long long ld_logits,
                                 float *out, float *sampling_loc_out, float *attn_weight_out, void *workspace,
                                 unsigned long long workspace_bytes, msda_stream_t stream)
{
    return msda::forward_prologue_body<float>("msda_forward_prologue_f32", {N, S, M, D, L, Lq, P},
                                              {value, spatial_shapes, level_start, sampling_offsets, attn_logits, out, (hipStream_t)stream,
                                               reference_points, sampling_loc_out, attn_weight_out, ld_offsets, ld_logits},
                                              {workspace, workspace_bytes});
}

int msda_backward_prologue_f32(const float *grad_out, const float *value, const int64_t *spatial_shapes,
                               const int64_t *level_start, const float *sampling_loc, const float *attn_weight, int N,
                               int S, int M, int D, int L, int Lq, int P, long long ld_grad_offsets,
                               long long ld_grad_logits, float *grad_value, float *grad_sampling_offsets,
                               float *grad_attn_logits, float *grad_reference_points, msda_stream_t stream)
{
    return msda_backward_prologue_ws_f32(grad_out, value, spatial_shapes, level_start, sampling_loc, attn_weight, N, S, M, D,
                                         L, Lq, P, ld_grad_offsets, ld_grad_logits, grad_value, grad_sampling_offsets,
                                         grad_attn_logits, grad_reference_points, nullptr, 0, 0, stream);
}

int msda_backward_prologue_ws_f32(const float *grad_out, const float *value, const int64_t *spatial_shapes,
                                  const int64_t *level_start, const float *sampling_loc, const float *attn_weight, int N,
                                  int S, int M, int D, int L, int Lq, int P, long long ld_grad_offsets,
                                  long long ld_grad_logits, float *grad_value, float *grad_sampling_offsets,
                                  float *grad_attn_logits, float *grad_reference_points, void *workspace,
                                  unsigned long long workspace_bytes, unsigned flags, msda_stream_t stream)
{
    return msda::backward_prologue_body<float>("msda_backward_prologue_f32", {N, S, M, D, L, Lq, P},
                                               {grad_out, value, spatial_shapes, level_start, sampling_loc, attn_weight, grad_value,
                                                grad_sampling_offsets, grad_attn_logits, (hipStream_t)stream, grad_reference_points,
                                                ld_grad_offsets, ld_grad_logits},
                                               {workspace, workspace_bytes, flags});
}

int msda_forward_prologue_bf16(const uint16_t *value, const int64_t *spatial_shapes, const int64_t *level_start,
                               const float *reference_points, const float *sampling_offsets, const float *attn_logits,
                               int N, int S, int M, int D, int L, int Lq, int P, long long ld_offsets, long long ld_logits,
                               uint16_t *out, float *sampling_loc_out, float *attn_weight_out, msda_stream_t stream)
{
    return msda_forward_prologue_ws_bf16(value, spatial_shapes, level_start, reference_points, sampling_offsets, attn_logits, N, S, M,
                                         D, L, Lq, P, ld_offsets, ld_logits, out, sampling_loc_out, attn_weight_out, nullptr, 0, stream);
}

int msda_forward_prologue_ws_bf16(const uint16_t *value, const int64_t *spatial_shapes, const int64_t *level_start,
                                  const float *reference_points, const float *sampling_offsets, const float *attn_logits,
                                  int N, int S, int M, int D, int L, int Lq, int P, long long ld_offsets, long long ld_logits,
                                  uint16_t *out, float *sampling_loc_out, float *attn_weight_out, void *workspace,
                                  unsigned long long workspace_bytes, msda_stream_t stream)
{
    return msda::forward_prologue_body<uint16_t>("msda_forward_prologue_bf16", {N, S, M, D, L, Lq, P},
                                                 {value, spatial_shapes, level_start, sampling_offsets, attn_logits, out, (hipStream_t)stream,
                                                  reference_points, sampling_loc_out, attn_weight_out, ld_offsets, ld_logits},
                                                 {workspace, workspace_bytes});
}

int msda_backward_prologue_bf16_gv32(const uint16_t *grad_out, const uint16_t *value, const int64_t *spatial_shapes,
                                     const int64_t *level_start, const float *sampling_loc, const float *attn_weight, int N,
                                     int S, int M, int D, int L, int Lq, int P, long long ld_grad_offsets,
                                     long long ld_grad_logits, float *grad_value, float *grad_sampling_offsets,
                                     float *grad_attn_logits, float *grad_reference_points, void *workspace,
                                     unsigned long long workspace_bytes, unsigned flags, msda_stream_t stream)
{
    return msda::backward_prologue_body<uint16_t>("msda_backward_prologue_bf16_gv32", {N, S, M, D, L, Lq, P},
                                                  {grad_out, value, spatial_shapes, level_start, sampling_loc, attn_weight, grad_value,
                                                   grad_sampling_offsets, grad_attn_logits, (hipStream_t)stream, grad_reference_points,
                                                   ld_grad_offsets, ld_grad_logits},
                                                  {workspace, workspace_bytes, flags});
}

unsigned long long msda_linear_wgrad_workspace_bytes(int M, int N, int K)
{
    if (M <= 0 || N <= 0 || K <= 0) return 0;
    return (unsigned long long)msda::linear_wgrad_workspace_bytes(M, N, K);
}

int msda_linear_wgrad_f32(const float *grad_out, const float *input, int M, int N, int K, float *grad_weight,
                          float *grad_bias, void *workspace, msda_stream_t stream)
{
    return msda_linear_wgrad_masked_f32(grad_out, input, nullptr, M, N, K, grad_weight, grad_bias, workspace, stream);
}

int msda_linear_wgrad_masked_f32(const float *grad_out, const float *input, const uint8_t *row_mask, int M, int N, int K,
                                 float *grad_weight, float *grad_bias, void *workspace, msda_stream_t stream)
{
    if (M < 0 || N <= 0 || K <= 0 || (N & 3) || (K & 3))
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_linear_wgrad_f32: need N, K > 0 and multiples of 4");
    if (grad_weight == nullptr || (M > 0 && (grad_out == nullptr || input == nullptr)))
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_linear_wgrad_f32: null device pointer");
    if (!msda::aligned_to(grad_out, 16) || !msda::aligned_to(input, 16) || !msda::aligned_to(workspace, 16))
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_linear_wgrad_f32: grad_out, input and workspace must be 16-byte aligned");
    msda::begin_call();
    if (M == 0) {
        hipError_t e = hipMemsetAsync(grad_weight, 0, sizeof(float) * (size_t)N * K, (hipStream_t)stream);
        if (e == hipSuccess && grad_bias) e = hipMemsetAsync(grad_bias, 0, sizeof(float) * (size_t)N, (hipStream_t)stream);
        return e == hipSuccess ? MSDA_OK : msda::set_error(MSDA_ERR_LAUNCH, hipGetErrorString(e));
    }
    return msda::launch_linear_wgrad(grad_out, input, row_mask, M, N, K, grad_weight, grad_bias,
                                     static_cast<float *>(workspace), (hipStream_t)stream);
}

int msda_linear_wgrad_multi(int count, const void *const *grad_out, const void *const *input, const int *operands_bf16,
                            const uint8_t *const *row_mask, const int *M, const int *N, const int *K, float *const *grad_weight,
                            float *const *grad_bias, void *const *workspace, msda_stream_t stream)
{
    if (count < 1 || count > 4 || !grad_out || !input || !M || !N || !K || !grad_weight || !workspace)
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_linear_wgrad_multi: 1..4 problems, non-null arrays");
    float *ws[4];
    for (int p = 0; p < count; ++p) {
        if (M[p] <= 0 || N[p] <= 0 || K[p] <= 0 || (N[p] & 3) || (K[p] & 3))
            return msda::set_error(MSDA_ERR_ARGUMENT, "msda_linear_wgrad_multi: need M, N, K > 0 and N, K multiples of 4");
        if (grad_weight[p] == nullptr || grad_out[p] == nullptr || input[p] == nullptr)
            return msda::set_error(MSDA_ERR_ARGUMENT, "msda_linear_wgrad_multi: null device pointer");
        // (bf16 operands: 8-byte alignment is what msda_linear_wgrad_masked_bf16 asks for)
        const size_t al = operands_bf16 && operands_bf16[p] ? 8 : 16;
        if (!msda::aligned_to(grad_out[p], al) || !msda::aligned_to(input[p], al) || !msda::aligned_to(workspace[p], 16))
            return msda::set_error(MSDA_ERR_ARGUMENT, "msda_linear_wgrad_multi: grad_out, input (16 bytes; bf16: 8) and workspace (16) alignment");
        if (msda::linear_wgrad_workspace_bytes(M[p], N[p], K[p]) > 0 && workspace[p] == nullptr)
            return msda::set_error(MSDA_ERR_ARGUMENT, "msda_linear_wgrad_multi: workspace required");
        ws[p] = static_cast<float *>(workspace[p]);
    }
    msda::begin_call();
    return msda::launch_linear_wgrad_multi(count, grad_out, input, operands_bf16, row_mask, M, N, K, grad_weight, grad_bias, ws,
                                           (hipStream_t)stream);
}

int msda_linear_wgrad_multi_f32(int count, const float *const *grad_out, const float *const *input, const uint8_t *const *row_mask,
                                const int *M, const int *N, const int *K, float *const *grad_weight, float *const *grad_bias,
                                void *const *workspace, msda_stream_t stream)
{
    return msda_linear_wgrad_multi(count, reinterpret_cast<const void *const *>(grad_out), reinterpret_cast<const void *const *>(input),
                                   nullptr, row_mask, M, N, K, grad_weight, grad_bias, workspace, stream);
}

int msda_linear_wgrad_masked_bf16(const uint16_t *grad_out, const uint16_t *input, const uint8_t *row_mask, int M, int N, int K,
                                  float *grad_weight, float *grad_bias, void *workspace, msda_stream_t stream)
{
    if (M < 0 || N <= 0 || K <= 0 || (N & 3) || (K & 3))
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_linear_wgrad_masked_bf16: need N, K > 0 and multiples of 4");
    if (grad_weight == nullptr || (M > 0 && (grad_out == nullptr || input == nullptr)))
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_linear_wgrad_masked_bf16: null device pointer");
    if (!msda::aligned_to(grad_out, 8) || !msda::aligned_to(input, 8) || !msda::aligned_to(workspace, 16))
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_linear_wgrad_masked_bf16: grad_out and input must be 8-byte, workspace "
                                                  "16-byte aligned");
    msda::begin_call();
    if (M == 0) {
        hipError_t e = hipMemsetAsync(grad_weight, 0, sizeof(float) * (size_t)N * K, (hipStream_t)stream);
        if (e == hipSuccess && grad_bias) e = hipMemsetAsync(grad_bias, 0, sizeof(float) * (size_t)N, (hipStream_t)stream);
        return e == hipSuccess ? MSDA_OK : msda::set_error(MSDA_ERR_LAUNCH, hipGetErrorString(e));
    }
    return msda::launch_linear_wgrad_bf16(grad_out, input, row_mask, M, N, K, grad_weight, grad_bias,
                                          static_cast<float *>(workspace), (hipStream_t)stream);
}

int msda_zero_masked_rows_f32(float *x, const uint8_t *row_mask, long long rows, int cols, msda_stream_t stream)
{
    if (rows < 0 || cols <= 0 || (cols & 3) || ((uintptr_t)x & 15))
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_zero_masked_rows_f32: need rows >= 0, cols > 0 and a multiple of 4, "
                                                  "16-byte aligned rows");
    if (rows > 0 && (x == nullptr || row_mask == nullptr))
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_zero_masked_rows_f32: null device pointer");
    if (rows > (1LL << 26) - 4) return msda::set_error(MSDA_ERR_ARGUMENT, "msda_zero_masked_rows_f32: too many rows");   // < 2^32 threads
    msda::begin_call();
    return msda::launch_zero_masked_rows(x, row_mask, rows, cols, (hipStream_t)stream);
}

static int check_linear_rows(const char *who, const void *a, const void *w, const void *bias, const void *out, long long rows,
                             int out_features, int in_features)
{
    if (rows < 0 || out_features <= 0 || in_features <= 0 || (out_features & 3) || (in_features & 3))
        return msda::set_error(MSDA_ERR_ARGUMENT, (std::string(who) + ": need rows >= 0 and out_features, in_features > 0 and "
                                                                       "multiples of 4").c_str());
    if (w == nullptr || (rows > 0 && (a == nullptr || out == nullptr)))
        return msda::set_error(MSDA_ERR_ARGUMENT, (std::string(who) + ": null device pointer").c_str());
    if (((uintptr_t)a | (uintptr_t)w | (uintptr_t)out | (uintptr_t)bias) & 15)
        return msda::set_error(MSDA_ERR_ARGUMENT, (std::string(who) + ": operands must be 16-byte aligned").c_str());
    return MSDA_OK;
}

int msda_linear_forward_f32(const float *input, const float *weight, const float *bias, const uint8_t *row_mask, long long rows,
                            int out_features, int in_features, float *output, msda_stream_t stream)
{
    if (int rc = check_linear_rows("msda_linear_forward_f32", input, weight, bias, output, rows, out_features, in_features)) return rc;
    msda::begin_call();
    return msda::launch_linear_forward(input, weight, bias, row_mask, rows, out_features, in_features, output, (hipStream_t)stream);
}

int msda_linear_dgrad_f32(const float *grad_out, const float *weight, const uint8_t *row_mask, long long rows, int out_features,
                          int in_features, float *grad_input, msda_stream_t stream)
{
    if (int rc = check_linear_rows("msda_linear_dgrad_f32", grad_out, weight, nullptr, grad_input, rows, out_features, in_features))
        return rc;
    msda::begin_call();
    return msda::launch_linear_dgrad(grad_out, weight, row_mask, rows, out_features, in_features, grad_input, (hipStream_t)stream);
}

static int check_layernorm_args(const char *who, long long rows, int d, const void *const *ptrs, int n)
{
    char buf[200];
    if (rows < 0 || d <= 0 || (d & 3) || d > 1024) {
        std::snprintf(buf, sizeof(buf), "%s: need rows >= 0 and a row width that is a multiple of 4 in [4, 1024]", who);
        return msda::set_error(MSDA_ERR_ARGUMENT, buf);
    }
    for (int i = 0; i < n; ++i)
        if (rows > 0 && (ptrs[i] == nullptr || ((uintptr_t)ptrs[i] & 15))) {
            std::snprintf(buf, sizeof(buf), "%s: null or not 16-byte aligned device pointer", who);
            return msda::set_error(MSDA_ERR_ARGUMENT, buf);
        }
    return MSDA_OK;
}

unsigned long long msda_add_layernorm_workspace_bytes(long long rows, int d)
{
    return (rows > 0 && d > 0) ? (unsigned long long)msda::add_layernorm_workspace_bytes(rows, d) : 0;
}

int msda_add_layernorm_forward_f32(const float *x, const float *residual, const float *gamma, const float *beta, long long rows,
                                   int d, float eps, float *y, float *mean, float *rstd, msda_stream_t stream)
{
    const void *ptrs[] = {x, gamma, beta, y};
    if (int rc = check_layernorm_args("msda_add_layernorm_forward_f32", rows, d, ptrs, 4)) return rc;
    if (rows > 0 && (mean == nullptr || rstd == nullptr || (residual && ((uintptr_t)residual & 15))))
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_add_layernorm_forward_f32: null mean / rstd or misaligned residual");
    msda::begin_call();
    if (rows == 0) return MSDA_OK;
    return msda::launch_add_layernorm_fwd(x, residual, gamma, beta, rows, d, eps, y, mean, rstd, (hipStream_t)stream);
}

int msda_add_layernorm_backward_f32(const float *grad_y, const float *x, const float *residual, const float *gamma,
                                    const float *mean, const float *rstd, long long rows, int d, float *grad_sum,
                                    float *grad_gamma, float *grad_beta, void *workspace, msda_stream_t stream)
{
    const void *ptrs[] = {grad_y, x, gamma, grad_sum, workspace};
    if (int rc = check_layernorm_args("msda_add_layernorm_backward_f32", rows, d, ptrs, 5)) return rc;
    if (grad_gamma == nullptr || grad_beta == nullptr || (rows > 0 && (mean == nullptr || rstd == nullptr)) ||
        (residual && ((uintptr_t)residual & 15)))
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_add_layernorm_backward_f32: null pointer or misaligned residual");
    msda::begin_call();
    if (rows == 0) {
        hipError_t e = hipMemsetAsync(grad_gamma, 0, sizeof(float) * (size_t)d, (hipStream_t)stream);
        if (e == hipSuccess) e = hipMemsetAsync(grad_beta, 0, sizeof(float) * (size_t)d, (hipStream_t)stream);
        return e == hipSuccess ? MSDA_OK : msda::set_error(MSDA_ERR_LAUNCH, hipGetErrorString(e));
    }
    return msda::launch_add_layernorm_bwd(grad_y, x, residual, gamma, mean, rstd, rows, d, grad_sum, grad_gamma, grad_beta,
                                          static_cast<float *>(workspace), (hipStream_t)stream);
}

// x fp32, residual bf16 (8-byte aligned rows: a bf16 projection output under autocast); the arithmetic of the fp32 entries
int msda_add_layernorm_forward_f32_bf16res(const float *x, const uint16_t *residual, const float *gamma, const float *beta,
                                           long long rows, int d, float eps, float *y, float *mean, float *rstd, msda_stream_t stream)
{
    const void *ptrs[] = {x, gamma, beta, y};
    if (int rc = check_layernorm_args("msda_add_layernorm_forward_f32_bf16res", rows, d, ptrs, 4)) return rc;
    if (rows > 0 && (mean == nullptr || rstd == nullptr || residual == nullptr || ((uintptr_t)residual & 7)))
        return msda::set_error(MSDA_ERR_ARGUMENT,
                               "msda_add_layernorm_forward_f32_bf16res: null mean / rstd / residual or residual not 8-byte aligned");
    msda::begin_call();
    if (rows == 0) return MSDA_OK;
    return msda::launch_add_layernorm_fwd_bf16res(x, residual, gamma, beta, rows, d, eps, y, mean, rstd, (hipStream_t)stream);
}

int msda_add_layernorm_backward_f32_bf16res(const float *grad_y, const float *x, const uint16_t *residual, const float *gamma,
                                            const float *mean, const float *rstd, long long rows, int d, float *grad_x,
                                            uint16_t *grad_residual, float *grad_gamma, float *grad_beta, void *workspace,
                                            msda_stream_t stream)
{
    const void *ptrs[] = {grad_y, x, gamma, grad_x, workspace};
    if (int rc = check_layernorm_args("msda_add_layernorm_backward_f32_bf16res", rows, d, ptrs, 5)) return rc;
    if (grad_gamma == nullptr || grad_beta == nullptr ||
        (rows > 0 && (mean == nullptr || rstd == nullptr || residual == nullptr || grad_residual == nullptr ||
                      ((uintptr_t)residual & 7) || ((uintptr_t)grad_residual & 7))))
        return msda::set_error(MSDA_ERR_ARGUMENT,
                               "msda_add_layernorm_backward_f32_bf16res: null pointer or residual / grad_residual not 8-byte aligned");
    msda::begin_call();
    if (rows == 0) {
        hipError_t e = hipMemsetAsync(grad_gamma, 0, sizeof(float) * (size_t)d, (hipStream_t)stream);
        if (e == hipSuccess) e = hipMemsetAsync(grad_beta, 0, sizeof(float) * (size_t)d, (hipStream_t)stream);
        return e == hipSuccess ? MSDA_OK : msda::set_error(MSDA_ERR_LAUNCH, hipGetErrorString(e));
    }
    return msda::launch_add_layernorm_bwd_bf16res(grad_y, x, residual, gamma, mean, rstd, rows, d, grad_x, grad_residual, grad_gamma,
                                                  grad_beta, static_cast<float *>(workspace), (hipStream_t)stream);
}

int msda_cast_bf16_multi_f32(int count, const float *const *src, uint16_t *const *dst, const long long *n, msda_stream_t stream)
{
    if (count < 1 || count > 4 || src == nullptr || dst == nullptr || n == nullptr)
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_cast_bf16_multi_f32: 1..4 segments");
    for (int k = 0; k < count; ++k)
        if (n[k] < 0 || (n[k] & 1) || (n[k] > 0 && (src[k] == nullptr || dst[k] == nullptr)) || ((uintptr_t)src[k] & 7) || ((uintptr_t)dst[k] & 3))
            return msda::set_error(MSDA_ERR_ARGUMENT, "msda_cast_bf16_multi_f32: element counts must be even, sources 8-byte and destinations 4-byte aligned");
    msda::begin_call();
    return msda::launch_cast_bf16_multi(count, src, dst, n, (hipStream_t)stream);
}

int msda_relu_dropout_backward_f32(float *grad, const float *act, float scale, long long n, msda_stream_t stream)
{
    if (n < 0 || (n & 3) || (n > 0 && (grad == nullptr || act == nullptr)) || (((uintptr_t)grad | (uintptr_t)act) & 15))
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_relu_dropout_backward_f32: n must be a multiple of 4 and both tensors 16-byte aligned");
    msda::begin_call();
    if (n == 0) return MSDA_OK;
    return msda::launch_relu_dropout_bwd(grad, act, scale, n, (hipStream_t)stream);
}

static int flatten_impl(const char *who, int L, float *const *src_levels, float *const *pos_levels, const float *level_embed,
                        const int *heights, const int *widths, int N, int C, float *src_flatten, float *pos_flatten, bool unflatten,
                        msda_stream_t stream, float *grad_level_embed = nullptr, void *workspace = nullptr,
                        unsigned long long *workspace_bytes_out = nullptr)
{
    char buf[200];
    if (L <= 0 || L > msda::kMaxLevels || N < 0 || C <= 0 || (C & 3) || heights == nullptr || widths == nullptr) {
        std::snprintf(buf, sizeof(buf), "%s: need 1 <= L <= %d, N >= 0, C > 0 and a multiple of 4, host arrays of H and W", who,
                      msda::kMaxLevels);
        return msda::set_error(MSDA_ERR_ARGUMENT, buf);
    }
    msda::FlattenPlan plan;
    plan.L = L;
    long long S = 0;
    for (int l = 0; l < L; ++l) {
        if (heights[l] <= 0 || widths[l] <= 0 || (long long)heights[l] * widths[l] > 0x3fffffffLL)
            return msda::set_error(MSDA_ERR_ARGUMENT, "msda flatten: level sizes must be positive");
        plan.src[l] = src_levels ? src_levels[l] : nullptr;
        plan.pos[l] = pos_levels ? pos_levels[l] : nullptr;
        if (N > 0 && ((src_flatten && plan.src[l] == nullptr) || (pos_flatten && plan.pos[l] == nullptr)))
            return msda::set_error(MSDA_ERR_ARGUMENT, "msda flatten: null level pointer");
        plan.hw[l] = heights[l] * widths[l];
        plan.start[l] = (int)S;
        plan.first_block[l] = 0;
        S += plan.hw[l];
    }
    if (S > 0x3fffffffLL) return msda::set_error(MSDA_ERR_ARGUMENT, "msda flatten: too many pixels");
    if (((uintptr_t)src_flatten & 15) || ((uintptr_t)pos_flatten & 15) || ((uintptr_t)level_embed & 15))
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda flatten: flattened tensors and level_embed must be 16-byte aligned");
    if (workspace_bytes_out) { *workspace_bytes_out = N > 0 ? msda::unflatten_workspace_bytes(plan, N, C) : 0; return MSDA_OK; }
    if (((uintptr_t)grad_level_embed & 15) || ((uintptr_t)workspace & 15))
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda unflatten: grad_level_embed and workspace must be 16-byte aligned");
    msda::begin_call();
    if (N == 0) {
        if (grad_level_embed) {
            const hipError_t e = hipMemsetAsync(grad_level_embed, 0, sizeof(float) * (size_t)L * C, (hipStream_t)stream);
            if (e != hipSuccess) return msda::set_error(MSDA_ERR_LAUNCH, hipGetErrorString(e));
        }
        return MSDA_OK;
    }
    return msda::launch_flatten_levels(plan, N, C, (int)S, level_embed, src_flatten, pos_flatten, unflatten, (hipStream_t)stream,
                                       grad_level_embed, static_cast<float *>(workspace));
}

int msda_flatten_levels_f32(int L, const float *const *src_levels, const float *const *pos_levels, const float *level_embed,
                            const int *heights, const int *widths, int N, int C, float *src_flatten, float *pos_flatten,
                            msda_stream_t stream)
{
    return flatten_impl("msda_flatten_levels_f32", L, const_cast<float *const *>(src_levels), const_cast<float *const *>(pos_levels),
                        level_embed, heights, widths, N, C, src_flatten, pos_flatten, false, stream);
}

int msda_unflatten_levels_f32(int L, float *const *grad_src_levels, float *const *grad_pos_levels, const int *heights,
                              const int *widths, int N, int C, const float *grad_src_flatten, const float *grad_pos_flatten,
                              float *grad_level_embed, void *workspace, msda_stream_t stream)
{
    return flatten_impl("msda_unflatten_levels_f32", L, grad_src_levels, grad_pos_levels, nullptr, heights, widths, N, C,
                        const_cast<float *>(grad_src_flatten), const_cast<float *>(grad_pos_flatten), true, stream,
                        grad_level_embed, workspace);
}

unsigned long long msda_unflatten_workspace_bytes(int L, const int *heights, const int *widths, int N, int C)
{
    unsigned long long n = 0;
    float *dummy[msda::kMaxLevels] = {};
    if (flatten_impl("msda_unflatten_workspace_bytes", L, dummy, dummy, nullptr, heights, widths, N, C, nullptr, nullptr, true, nullptr,
                     nullptr, nullptr, &n) != MSDA_OK)
        return 0;
    return n;
}

const char *msda_last_error(void) { return msda::g_err; }

int msda_version(void) { return MSDA_ABI_VERSION; }

int msda_path_for(int elem_bytes, int M, int D, int L, int P)
{
    // N, S, Lq only matter through the int32-offset limits; probe with small ones.
    return ((elem_bytes == 4 || elem_bytes == 2) && msda::use_d32({1, 1, M, D, L, 1, P})) ? MSDA_PATH_D32 : MSDA_PATH_GENERIC;
}

void msda_force_path(int path) { msda::g_force_path = path; }

unsigned long long msda_launch_count(void) { return msda::launch_checks(); }

int msda_describe_plan(int row_bytes, int grad_value_bytes, int N, int S, int M, int D, int L, int Lq, int P, unsigned flags,
                       int has_workspace, char *buf, int buf_len)
{
    if (!buf || buf_len <= 0) return 0;
    buf[0] = 0;
    const msda::OpGeom g{N, S, M, D, L, Lq, P};
    if (!g.nonempty()) return 0;
    if ((row_bytes != 4 && row_bytes != 2) || !msda::use_d32(g)) {
        const int k = snprintf(buf, (size_t)buf_len, "generic");
        return k < buf_len ? k : buf_len - 1;
    }
    const bool prologue = (flags & MSDA_FLAG_PROLOGUE) != 0;
    if (prologue && !msda::prologue_supported(g)) {
        const int k = snprintf(buf, (size_t)buf_len, "prologue unsupported");
        return k < buf_len ? k : buf_len - 1;
    }
    const int k = msda::describe_plan(row_bytes, row_bytes == 4 ? 4 : grad_value_bytes, g, prologue,
                                      msda::OpOptions(nullptr, has_workspace != 0, flags), buf, buf_len);
    return k < buf_len ? k : buf_len - 1;
}

/* ---- two-stage query selection (msda_two_stage.hip) ---- */
static bool misaligned16(const void *p) { return ((uintptr_t)p & 15) != 0; }

int msda_two_stage_proposals_f32(const float *memory, const uint8_t *padding_mask, int N, int S, int C, int L, const int *heights,
                                 const int *widths, const float *learnedxy, float *proposals, float *memory_out, uint8_t *row_mask,
                                 msda_stream_t stream)
{
    if (N < 0 || S < 0 || C <= 0 || (C & 3) || L <= 0 || L > msda::kMaxLevels)
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_two_stage_proposals_f32: need N, S >= 0, C > 0 and a multiple of 4, "
                                                  "1 <= L <= 16");
    if (heights == nullptr || widths == nullptr)
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_two_stage_proposals_f32: null level table");
    long long total = 0;
    for (int l = 0; l < L; ++l) {
        if (heights[l] <= 0 || widths[l] <= 0) return msda::set_error(MSDA_ERR_ARGUMENT, "msda_two_stage_proposals_f32: empty level");
        total += (long long)heights[l] * widths[l];
    }
    if (total != S) return msda::set_error(MSDA_ERR_ARGUMENT, "msda_two_stage_proposals_f32: S is not the sum of H_l * W_l");
    if ((long long)N * S * (C > 42 ? C : 42) >= (1LL << 31))
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_two_stage_proposals_f32: tensors beyond 2^31 elements");
    if (N > 0 && S > 0 && (memory == nullptr || padding_mask == nullptr || proposals == nullptr || memory_out == nullptr ||
                           row_mask == nullptr))
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_two_stage_proposals_f32: null device pointer");
    if (misaligned16(memory) || misaligned16(memory_out))
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_two_stage_proposals_f32: memory rows must be 16-byte aligned");
    msda::begin_call();
    return msda::launch_two_stage_proposals(memory, padding_mask, N, S, C, L, heights, widths, learnedxy, proposals, memory_out,
                                            row_mask, (hipStream_t)stream);
}

int msda_two_stage_select_supported(int S, int K, int Q) { return S > 0 && S <= msda::kSelMaxRows && K > 0 && Q >= 0 && Q <= S; }

int msda_two_stage_select_f32(const float *cls, const float *hand, const float *obj, const float *proposals, int N, int S, int K,
                              int Q, int hand_class0, int hand_class1, int64_t *topk, float *refpoint_unsig,
                              float *reference_points, msda_stream_t stream)
{
    if (N < 0 || S <= 0 || K <= 0 || Q < 0)
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_two_stage_select_f32: need N >= 0, S > 0, K > 0, Q >= 0");
    if (Q > S) return msda::set_error(MSDA_ERR_ARGUMENT, "msda_two_stage_select_f32: selected index k out of range (Q > S)");
    if (S > msda::kSelMaxRows) return msda::set_error(MSDA_ERR_ARGUMENT, "msda_two_stage_select_f32: S above 8192 rows per frame");
    if ((long long)N * S * (K > 42 ? K : 42) >= (1LL << 31))
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_two_stage_select_f32: tensors beyond 2^31 elements");
    if (N > 0 && Q > 0 && (cls == nullptr || hand == nullptr || obj == nullptr || proposals == nullptr ||
                           refpoint_unsig == nullptr || reference_points == nullptr))
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_two_stage_select_f32: null device pointer");
    msda::begin_call();
    return msda::launch_two_stage_select(cls, hand, obj, proposals, N, S, K, Q, hand_class0, hand_class1, topk, refpoint_unsig,
                                         reference_points, (hipStream_t)stream);
}

int msda_proposal_pos_embed_f32(const float *refpoint_unsig, const float *dim_t, long long M, float *pe, msda_stream_t stream)
{
    if (M < 0 || M > (1LL << 31) / 5376) return msda::set_error(MSDA_ERR_ARGUMENT, "msda_proposal_pos_embed_f32: need 0 <= M < 399458");
    if (M > 0 && (refpoint_unsig == nullptr || dim_t == nullptr || pe == nullptr))
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_proposal_pos_embed_f32: null device pointer");
    if (misaligned16(pe)) return msda::set_error(MSDA_ERR_ARGUMENT, "msda_proposal_pos_embed_f32: pe must be 16-byte aligned");
    msda::begin_call();
    return msda::launch_pe(refpoint_unsig, dim_t, M, pe, (hipStream_t)stream);
}

int msda_proposal_pos_linear_relu_f32(const float *refpoint_unsig, const float *dim_t, const float *weight, const float *bias,
                                      long long M, int out_features, float *y, msda_stream_t stream)
{
    if (M < 0 || out_features <= 0 || (out_features & 3) || M > (1LL << 31) / 5376)
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_proposal_pos_linear_relu_f32: need 0 <= M < 399458, out_features > 0 and "
                                                  "a multiple of 4");
    if (weight == nullptr || dim_t == nullptr || (M > 0 && (refpoint_unsig == nullptr || y == nullptr)))
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_proposal_pos_linear_relu_f32: null device pointer");
    if (misaligned16(weight)) return msda::set_error(MSDA_ERR_ARGUMENT, "msda_proposal_pos_linear_relu_f32: weight must be 16-byte aligned");
    msda::begin_call();
    return msda::launch_pe_linear_relu(refpoint_unsig, dim_t, weight, bias, M, out_features, y, (hipStream_t)stream);
}

/* ---- the AssemblyHands transformer (msda_assembly.hip) ---- */
int msda_assembly_refine_f32(const float *reference_points, int width, const float *cls, int K, const float *keypoints, long long M,
                             float *out, msda_stream_t stream)
{
    if (M < 0 || (width != 2 && width != 42) || K <= 0)
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_assembly_refine_f32: need M >= 0, width 2 or 42 and K > 0");
    if (M * (K > 63 ? K : 63) >= (1LL << 31))
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_assembly_refine_f32: tensors beyond 2^31 elements");
    if (M > 0 && (reference_points == nullptr || cls == nullptr || keypoints == nullptr || out == nullptr))
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_assembly_refine_f32: null device pointer");
    msda::begin_call();
    return msda::launch_assembly_refine(reference_points, width, cls, K, keypoints, M, out, (hipStream_t)stream);
}

/* ---- the DINO decoder's query positions and refinement (msda_dino.hip) ---- */
static const char *dino_rows_error(int width, int N, long long M)
{
    if (width != 2 && width != 42) return "width must be 2 or 42";
    if (N <= 0 || M < 0 || M % N != 0) return "need N > 0, M >= 0 and M a multiple of N (rows are sequence-first)";
    if (M * 256 >= (1LL << 31)) return "tensors beyond 2^31 elements";
    return nullptr;
}

int msda_dino_sine_embed_f32(const float *ref, int width, const float *valid_xy, int N, long long M, const float *dim_t, float *pe,
                             msda_stream_t stream)
{
    if (dino_rows_error(width, N, M)) return msda::set_error(MSDA_ERR_ARGUMENT, dino_rows_error(width, N, M));
    if (dim_t == nullptr || (M > 0 && (ref == nullptr || pe == nullptr)))
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_dino_sine_embed_f32: null device pointer");
    if (misaligned16(pe)) return msda::set_error(MSDA_ERR_ARGUMENT, "msda_dino_sine_embed_f32: pe must be 16-byte aligned");
    msda::begin_call();
    return msda::launch_dino_sine_embed(ref, width, valid_xy, N, M, dim_t, pe, (hipStream_t)stream);
}

int msda_dino_query_pos_supported(int width, int N, long long M, int hidden, int out_features)
{
    return dino_rows_error(width, N, M) == nullptr && hidden == 256 && out_features == 256;
}

int msda_dino_query_pos_forward_f32(const float *ref, int width, const float *valid_xy, int N, long long M, const float *dim_t,
                                    const float *w1, const float *b1, const float *w2, const float *b2, float *h, float *y,
                                    msda_stream_t stream)
{
    if (dino_rows_error(width, N, M)) return msda::set_error(MSDA_ERR_ARGUMENT, dino_rows_error(width, N, M));
    if (dim_t == nullptr || w1 == nullptr || b1 == nullptr || w2 == nullptr || b2 == nullptr ||
        (M > 0 && (ref == nullptr || h == nullptr || y == nullptr)))
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_dino_query_pos_forward_f32: null device pointer");
    if (misaligned16(w1) || misaligned16(w2))
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_dino_query_pos_forward_f32: weights must be 16-byte aligned");
    msda::begin_call();
    return msda::launch_dino_query_pos(ref, width, valid_xy, N, M, dim_t, w1, b1, w2, b2, h, y, (hipStream_t)stream);
}

int msda_dino_refine_forward_f32(const float *ref, const float *cls, int K, const float *delta_key, const float *delta_obj, int hand0,
                                 int hand1, long long M, float *out, uint8_t *code, msda_stream_t stream)
{
    if (M < 0 || K < 1) return msda::set_error(MSDA_ERR_ARGUMENT, "msda_dino_refine_forward_f32: need M >= 0 and K >= 1");
    if (M * (K > 42 ? K : 42) >= (1LL << 31))
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_dino_refine_forward_f32: tensors beyond 2^31 elements");
    if (M > 0 && (ref == nullptr || cls == nullptr || delta_key == nullptr || delta_obj == nullptr || out == nullptr || code == nullptr))
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_dino_refine_forward_f32: null device pointer");
    msda::begin_call();
    return msda::launch_dino_refine_fwd(ref, cls, K, delta_key, delta_obj, hand0, hand1, M, out, code, (hipStream_t)stream);
}

int msda_dino_refine_backward_f32(const float *grad_out, const float *out, const uint8_t *code, long long M, float *grad_key,
                                  float *grad_obj, msda_stream_t stream)
{
    if (M < 0 || M * 42 >= (1LL << 31))
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_dino_refine_backward_f32: need 0 <= M and M * 42 < 2^31");
    if (M > 0 && (grad_out == nullptr || out == nullptr || code == nullptr))
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_dino_refine_backward_f32: null device pointer");
    msda::begin_call();
    return msda::launch_dino_refine_bwd(grad_out, out, code, M, grad_key, grad_obj, (hipStream_t)stream);
}

/* ---- DINO's two-stage query selection (msda_dino_select.hip) ---- */
int msda_dino_select_supported(int S, int K, int Q, int C)
{
    return S >= 1 && S <= msda::kDinoSelMaxRows && Q >= 1 && Q <= S && Q <= msda::kDinoSelMaxQueries && K >= 1 && K <= 256 &&
           C >= 4 && (C & 3) == 0 && C <= 2048;
}

unsigned long long msda_dino_select_workspace_bytes(int N, int S)
{
    if (N <= 0 || S <= 0) return 0;
    return (unsigned long long)msda::dino_select_workspace_bytes(N, S);
}

int msda_dino_select_forward_f32(const float *cls, const float *memory, const float *proposals, int N, int S, int K, int Q, int C,
                                 int hand_class0, int hand_class1, int64_t *topk, int32_t *slot, float *tgt, float *prop_sel,
                                 uint8_t *code, void *workspace, msda_stream_t stream)
{
    if (N < 0 || N > msda::kDinoSelMaxFrames)
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_dino_select_forward_f32: need 0 <= N <= 65535");
    if (S >= 1 && Q > S) return msda::set_error(MSDA_ERR_ARGUMENT, "msda_dino_select_forward_f32: selected index k out of range (Q > S)");
    if (!msda_dino_select_supported(S, K, Q, C))
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_dino_select_forward_f32: need 1 <= Q <= min(S, 2048), S <= 2^20, 1 <= K <= 256 "
                                                  "and C a multiple of 4 in 4..2048");
    const int widest = C > K ? (C > 42 ? C : 42) : (K > 42 ? K : 42);
    if ((long long)N * S * widest >= (1LL << 31))
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_dino_select_forward_f32: tensors beyond 2^31 elements");
    if (N == 0) return MSDA_OK;
    if (cls == nullptr || memory == nullptr || proposals == nullptr || topk == nullptr || slot == nullptr || tgt == nullptr ||
        prop_sel == nullptr || code == nullptr || workspace == nullptr)
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_dino_select_forward_f32: null device pointer");
    if (misaligned16(memory) || misaligned16(tgt) || misaligned16(workspace))
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_dino_select_forward_f32: memory, tgt and workspace must be 16-byte aligned");
    msda::begin_call();
    return msda::launch_dino_select_fwd(cls, memory, proposals, N, S, K, Q, C, hand_class0, hand_class1, topk, slot, tgt, prop_sel,
                                        code, workspace, (hipStream_t)stream);
}

int msda_dino_select_backward_f32(const int32_t *slot, const float *grad_tgt, int N, int S, int Q, int C, float *grad_memory,
                                  msda_stream_t stream)
{
    if (N < 0 || S < 1 || Q < 1 || Q > S || Q > msda::kDinoSelMaxQueries || C < 4 || (C & 3) || C > 2048)
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_dino_select_backward_f32: need N >= 0, 1 <= Q <= min(S, 2048) and C a multiple "
                                                  "of 4 in 4..2048");
    if ((long long)N * S * C >= (1LL << 31))
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_dino_select_backward_f32: tensors beyond 2^31 elements");
    if (N == 0) return MSDA_OK;
    if (slot == nullptr || grad_tgt == nullptr || grad_memory == nullptr)
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_dino_select_backward_f32: null device pointer");
    if (misaligned16(grad_tgt) || misaligned16(grad_memory))
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_dino_select_backward_f32: grad_tgt and grad_memory must be 16-byte aligned");
    msda::begin_call();
    return msda::launch_dino_select_bwd(slot, grad_tgt, N, S, Q, C, grad_memory, (hipStream_t)stream);
}

/* ---- DINO's contrastive-denoising queries (msda_cdn.hip) ---- */
int msda_cdn_supported(int hidden, int width, long long rows_book, long long E)
{
    if (hidden < 4 || hidden > 1024 || (hidden & 3) || width < 1 || width > 64 || rows_book < 1 || E < 0) return 0;
    if (E >= (1LL << 31) || 2 * E * (1 + (long long)width) >= (1LL << 32)) return 0;      /* the last key-noise counter */
    return rows_book * hidden < (1LL << 31);
}

int msda_cdn_prepare_forward_f32(const int64_t *labels, const int64_t *offsets, const float *keypoints, const float *weight,
                                 const long long *seed, int B, long long T, int width, int hidden, long long rows_book,
                                 int single_pad, int groups, int num_classes, unsigned flip_threshold, float key_noise_scale,
                                 float *input_query_label, float *input_query_key, int32_t *noised_labels, float *key_debug,
                                 msda_stream_t stream)
{
    if (B < 0 || T < 0 || single_pad < 0 || groups < 1 || num_classes < 1 || !(key_noise_scale >= 0.f))
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_cdn_prepare_forward_f32: need B, T, single_pad >= 0, groups, num_classes >= 1 "
                                                  "and key_noise_scale >= 0");
    if ((long long)groups * T >= (1LL << 30) || !msda_cdn_supported(hidden, width, rows_book, 2LL * groups * T))
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_cdn_prepare_forward_f32: outside msda_cdn_supported (hidden a multiple of 4 in "
                                                  "4..1024, width 1..64, counters below 2^32)");
    if (num_classes > rows_book)
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_cdn_prepare_forward_f32: num_classes exceeds the embedding's rows");
    const long long rows = 2LL * single_pad * groups * B;
    if (2LL * single_pad * groups >= (1LL << 31) || rows * (hidden > width ? hidden : width) >= (1LL << 31))
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_cdn_prepare_forward_f32: tensors beyond 2^31 elements");
    if (rows == 0) return MSDA_OK;
    if (offsets == nullptr || weight == nullptr || input_query_label == nullptr || input_query_key == nullptr ||
        noised_labels == nullptr || (T > 0 && (labels == nullptr || keypoints == nullptr)))
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_cdn_prepare_forward_f32: null device pointer");
    if ((flip_threshold != 0u || key_noise_scale > 0.f) && seed == nullptr)
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_cdn_prepare_forward_f32: draws need a seed");
    if (misaligned16(weight) || misaligned16(input_query_label))
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_cdn_prepare_forward_f32: weight and input_query_label must be 16-byte aligned");
    msda::begin_call();
    return msda::launch_cdn_prepare_fwd(labels, offsets, keypoints, weight, seed, B, T, width, hidden, rows_book, single_pad, groups,
                                        num_classes, flip_threshold, key_noise_scale, input_query_label, input_query_key,
                                        noised_labels, key_debug, (hipStream_t)stream);
}

int msda_cdn_prepare_backward_f32(const float *grad_label, const int32_t *noised_labels, long long rows, int hidden,
                                  long long rows_book, float *grad_weight, msda_stream_t stream)
{
    if (rows < 0 || !msda_cdn_supported(hidden, 1, rows_book, 0) || rows * hidden >= (1LL << 31))
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_cdn_prepare_backward_f32: need rows >= 0, hidden a multiple of 4 in 4..1024, "
                                                  "rows_book >= 1 and tensors below 2^31 elements");
    if (grad_weight == nullptr || (rows > 0 && (grad_label == nullptr || noised_labels == nullptr)))
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_cdn_prepare_backward_f32: null device pointer");
    if (misaligned16(grad_label) || misaligned16(grad_weight))
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_cdn_prepare_backward_f32: grad_label and grad_weight must be 16-byte aligned");
    msda::begin_call();
    return msda::launch_cdn_prepare_bwd(grad_label, noised_labels, rows, hidden, rows_book, grad_weight, (hipStream_t)stream);
}

int msda_assembly_proposals_f32(const float *memory, long long memory_frame_stride, const uint8_t *padding_mask,
                                long long mask_frame_stride, int N, int H, int W, int C, float *proposals, float *memory_out,
                                uint8_t *row_mask, msda_stream_t stream)
{
    if (N < 0 || H <= 0 || W <= 0 || C <= 0 || (C & 3))
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_assembly_proposals_f32: need N >= 0, H, W > 0 and C > 0 a multiple of 4");
    const long long rows = (long long)H * W;
    if (memory_frame_stride < rows * C || (memory_frame_stride & 3) || mask_frame_stride < rows)
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_assembly_proposals_f32: frame strides must cover H*W rows and the memory "
                                                  "stride be a multiple of 4");
    if ((long long)N * memory_frame_stride >= (1LL << 31) || (long long)N * rows * C >= (1LL << 31) ||
        (long long)N * mask_frame_stride >= (1LL << 31))
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_assembly_proposals_f32: tensors beyond 2^31 elements");
    if (N > 0 && (memory == nullptr || padding_mask == nullptr || proposals == nullptr || memory_out == nullptr || row_mask == nullptr))
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_assembly_proposals_f32: null device pointer");
    if (misaligned16(memory) || misaligned16(memory_out))
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_assembly_proposals_f32: memory rows must be 16-byte aligned");
    msda::begin_call();
    return msda::launch_assembly_level_proposals(memory, memory_frame_stride, padding_mask, mask_frame_stride, N, H, W, C, proposals,
                                                 memory_out, row_mask, (hipStream_t)stream);
}

int msda_assembly_select_f32(const float *cls, const float *hand, const float *obj, int N, int S, int K, int obj_first, int obj_last,
                             int left, int right, int64_t *indices, float *reference_points, msda_stream_t stream)
{
    if (N < 0 || S <= 0 || K <= 0)
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_assembly_select_f32: need N >= 0, S > 0 and K > 0");
    if (obj_first < 0 || obj_last < obj_first || obj_last - obj_first + 1 > msda::kAssemblySelMaxObj)
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_assembly_select_f32: need 0 <= obj_first <= obj_last and at most 14 object "
                                                  "classes");
    if (obj_last >= K || left < 0 || left >= K || right < 0 || right >= K)
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_assembly_select_f32: class index out of range for K classes");
    if ((long long)N * S * (K > 63 ? K : 63) >= (1LL << 31))
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_assembly_select_f32: tensors beyond 2^31 elements");
    if (N > 0 && (cls == nullptr || hand == nullptr || obj == nullptr || reference_points == nullptr))
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_assembly_select_f32: null device pointer");
    msda::begin_call();
    return msda::launch_assembly_select(cls, hand, obj, N, S, K, obj_first, obj_last, left, right, indices, reference_points,
                                        (hipStream_t)stream);
}

/* ---- what the Hungarian matchers and the set criteria share: refusals and the binding of the prediction sets ---- */
// `who`: an entry's name, or the prefix ("msda_match", ...) of a message that a family's entries share.  The entries differ
// in what they check between the shared conditions, so each condition is a function that an entry calls in its own place.
static int refuse_set(const char *who, const char *fmt, ...)
{
    char buf[256];
    const int n = std::snprintf(buf, sizeof(buf), "%s: ", who);
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf + n, sizeof(buf) - n, fmt, ap);
    va_end(ap);
    return msda::set_error(MSDA_ERR_ARGUMENT, buf);
}

static int check_set_range(const char *who, int sets, int bs, int bs_min)
{
    if (sets < 1 || sets > msda::kMatchMaxSets || bs < bs_min || bs > msda::kMatchMaxQueries)
        return refuse_set(who, "need 1 <= sets <= %d and %d <= bs <= %d", msda::kMatchMaxSets, bs_min, msda::kMatchMaxQueries);
    return MSDA_OK;
}

// D >= 1 (and <= d_max when that is not 0) exactly when there are target keypoints
static int check_target_dim(const char *who, bool has_kp, int D, int d_max)
{
    if (has_kp ? (D < 1 || (d_max && D > d_max)) : D != 0) {
        if (d_max) return refuse_set(who, "need 1 <= D <= %d with target keypoints, D = 0 without", d_max);
        return refuse_set(who, "need D >= 1 with target keypoints, D = 0 without");
    }
    return MSDA_OK;
}

// the 2^31-element bounds: the targets' tensors, and one set's largest prediction tensor
static bool targets_beyond_2g(long long n_targets, int D) { return n_targets < 0 || n_targets * (D > 1 ? D : 1) >= (1LL << 31); }
static bool preds_beyond_2g(int bs, int Q, int K, int D) { return (long long)bs * Q * (K > D ? K : D) >= (1LL << 31); }
static int refuse_beyond_2g(const char *family) { return refuse_set(family, "tensors beyond 2^31 elements"); }

extern "C++" {   // templates over const float (predictions) and float (gradients)
// Set s's pointers into `out`; false when one that is wanted is null.  An array that is not wanted is not read.
template <class T>
static bool bind_set(int s, T *const *logits, T *const *hand, T *const *obj, bool want_hand, bool want_obj,
                     msda::PredSets<T> &out)
{
    out.logits[s] = logits[s];
    out.hand[s] = want_hand ? hand[s] : nullptr;
    out.obj[s] = want_obj ? obj[s] : nullptr;
    return out.logits[s] != nullptr && (!want_hand || out.hand[s] != nullptr) && (!want_obj || out.obj[s] != nullptr);
}

// Every set's; `null_msg` is the family's whole message for a null array or a null pointer in one.
template <class T>
static int bind_sets(const char *null_msg, int sets, T *const *logits, T *const *hand, T *const *obj, bool want_hand,
                     bool want_obj, msda::PredSets<T> &out)
{
    out = {};
    if (logits == nullptr || (want_hand && hand == nullptr) || (want_obj && obj == nullptr))
        return msda::set_error(MSDA_ERR_ARGUMENT, null_msg);
    for (int s = 0; s < sets; ++s)
        if (!bind_set(s, logits, hand, obj, want_hand, want_obj, out)) return msda::set_error(MSDA_ERR_ARGUMENT, null_msg);
    return MSDA_OK;
}
}   // extern "C++"

/* ---- the Hungarian matchers (msda_matcher.hip) ---- */
static const char kMatchNull[] = "msda_match: null device pointer";
static int check_match(const char *who, int sets, int bs, int Q, int K, int D, bool has_kp, const int64_t *labels,
                       const int64_t *offsets, long long n_targets, int t_max, const int64_t *out)
{
    int rc = check_set_range(who, sets, bs, 0);
    if (rc != MSDA_OK) return rc;
    if (Q < 1 || Q > msda::kMatchMaxQueries || K < 1 || t_max < 0 || t_max > msda::kMatchMaxTargets)
        return refuse_set(who, "need 1 <= Q <= %d, K >= 1 and 0 <= t_max <= %d", msda::kMatchMaxQueries, msda::kMatchMaxTargets);
    rc = check_target_dim(who, has_kp, D, msda::kMatchMaxDim);
    if (rc != MSDA_OK) return rc;
    if (targets_beyond_2g(n_targets, D) || preds_beyond_2g(bs, Q, K, D)) return refuse_beyond_2g("msda_match");
    if (bs > 0 && (offsets == nullptr || out == nullptr || (n_targets > 0 && labels == nullptr)))
        return msda::set_error(MSDA_ERR_ARGUMENT, kMatchNull);
    return MSDA_OK;
}

int msda_match_arctic_f32(const float *const *pred_logits, const float *const *pred_hand_key, const float *const *pred_obj_key,
                          int sets, int bs, int Q, int K, int D, const int64_t *labels, const float *keypoints,
                          const int64_t *offsets, long long n_targets, const int32_t *is_valid, int t_max, float cost_class,
                          float cost_keypoint, int64_t *out, float *cost_debug, msda_stream_t stream)
{
    const bool has_kp = keypoints != nullptr;
    int rc = check_match("msda_match_arctic_f32", sets, bs, Q, K, D, has_kp, labels, offsets, n_targets, t_max, out);
    if (rc != MSDA_OK) return rc;
    if (bs > 0 && is_valid == nullptr) return msda::set_error(MSDA_ERR_ARGUMENT, kMatchNull);
    msda::PredSets<const float> ms;
    rc = bind_sets(kMatchNull, sets, pred_logits, pred_hand_key, pred_obj_key, has_kp, has_kp, ms);
    if (rc != MSDA_OK) return rc;
    msda::begin_call();
    return msda::launch_match(ms, sets, bs, Q, K, D, {labels, keypoints, offsets, n_targets, is_valid, t_max}, cost_class,
                              cost_keypoint, out, cost_debug, (hipStream_t)stream);
}

int msda_match_assembly_f32(const float *const *pred_logits, const float *const *pred_keypoints, int sets, int bs, int Q, int K,
                            int D, const int64_t *labels, const float *keypoints, const int64_t *offsets, long long n_targets,
                            int t_max, float cost_class, float cost_keypoint, int64_t *out, float *cost_debug,
                            msda_stream_t stream)
{
    int rc = check_match("msda_match_assembly_f32", sets, bs, Q, K, D, true, labels, offsets, n_targets, t_max, out);
    if (rc != MSDA_OK) return rc;
    if (bs > 0 && n_targets > 0 && keypoints == nullptr) return msda::set_error(MSDA_ERR_ARGUMENT, kMatchNull);
    msda::PredSets<const float> ms;   // the one keypoint head is both the hand and the object head
    rc = bind_sets(kMatchNull, sets, pred_logits, pred_keypoints, pred_keypoints, true, true, ms);
    if (rc != MSDA_OK) return rc;
    msda::begin_call();
    return msda::launch_match(ms, sets, bs, Q, K, D, {labels, keypoints, offsets, n_targets, nullptr, t_max}, cost_class,
                              cost_keypoint, out, cost_debug, (hipStream_t)stream);
}

int msda_lsap_f32(const float *cost, int B, int Q, int T, int64_t *out, msda_stream_t stream)
{
    const int lo = Q < T ? Q : T, hi = Q < T ? T : Q;
    if (B < 0 || B > 65535 || Q < 1 || T < 0 || lo > msda::kMatchMaxTargets || hi > msda::kMatchMaxQueries)
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_lsap_f32: need 0 <= B <= 65535, Q >= 1, T >= 0, min(Q, T) <= 16 and "
                                                  "max(Q, T) <= 1024");
    if (B > 0 && (out == nullptr || (T > 0 && cost == nullptr)))
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_lsap_f32: null device pointer");
    msda::begin_call();
    return msda::launch_lsap(cost, B, Q, T, out, (hipStream_t)stream);
}

/* ---- the set criteria's matched losses (msda_criterion.hip) ---- */
static const char kCritNull[] = "msda_criterion: null pointer";
static int check_criterion(const char *who, int kind, const float *const *pred_logits, const float *const *pred_hand_key,
                           const float *const *pred_obj_key, int sets, int bs, int Q, int K, int D, const int64_t *match,
                           int t_max, const int64_t *labels, const float *keypoints, const int64_t *offsets,
                           long long n_targets, const int32_t *is_valid, const uint8_t *joint_valid,
                           unsigned long long hand_mask, const float *num_boxes, float focal_alpha, msda::CritArgs &a,
                           msda::PredSets<const float> &p)
{
    if (kind != MSDA_CRITERION_ARCTIC && kind != MSDA_CRITERION_ASSEMBLY)
        return refuse_set(who, "kind must be 0 (ARCTIC) or 1 (AssemblyHands)");
    int rc = check_set_range(who, sets, bs, 1);
    if (rc != MSDA_OK) return rc;
    if (Q < 1 || K < 1 || t_max < 0 || t_max > msda::kMatchMaxTargets || D < 0)
        return refuse_set(who, "need Q >= 1, K >= 1, D >= 0 and 0 <= t_max <= %d", msda::kMatchMaxTargets);
    const bool has_kp = keypoints != nullptr, arctic = kind == MSDA_CRITERION_ARCTIC;
    rc = check_target_dim(who, has_kp, D, 0);
    if (rc != MSDA_OK) return rc;
    if (targets_beyond_2g(n_targets, D) || preds_beyond_2g(bs, Q, K, D)) return refuse_beyond_2g("msda_criterion");
    if (match == nullptr || offsets == nullptr || num_boxes == nullptr || (n_targets > 0 && labels == nullptr)
        || (arctic && is_valid == nullptr) || (has_kp && !arctic && joint_valid == nullptr))
        return msda::set_error(MSDA_ERR_ARGUMENT, kCritNull);
    rc = bind_sets(kCritNull, sets, pred_logits, pred_hand_key, pred_obj_key, has_kp, has_kp && arctic, p);
    if (rc != MSDA_OK) return rc;
    a = {};
    a.kind = kind;
    a.sets = sets;
    a.bs = bs;
    a.Q = Q;
    a.K = K;
    a.D = D;
    a.match = match;
    a.tg = {labels, keypoints, offsets, n_targets, arctic ? is_valid : nullptr, t_max};
    a.joint_valid = !arctic && has_kp ? joint_valid : nullptr;
    a.hand_mask = hand_mask;
    a.num_boxes = num_boxes;
    a.alpha = focal_alpha;
    return MSDA_OK;
}

int msda_criterion_fwd_f32(int kind, const float *const *pred_logits, const float *const *pred_hand_key,
                           const float *const *pred_obj_key, int sets, int bs, int Q, int K, int D, const int64_t *match,
                           int t_max, const int64_t *labels, const float *keypoints, const int64_t *offsets,
                           long long n_targets, const int32_t *is_valid, const uint8_t *joint_valid,
                           unsigned long long hand_mask, const float *num_boxes, float focal_alpha, float *losses,
                           int32_t *stats, msda_stream_t stream)
{
    msda::CritArgs a;
    msda::PredSets<const float> p;
    int rc = check_criterion("msda_criterion_fwd_f32", kind, pred_logits, pred_hand_key, pred_obj_key, sets, bs, Q, K, D, match,
                             t_max, labels, keypoints, offsets, n_targets, is_valid, joint_valid, hand_mask, num_boxes,
                             focal_alpha, a, p);
    if (rc != MSDA_OK) return rc;
    if (losses == nullptr || stats == nullptr) return msda::set_error(MSDA_ERR_ARGUMENT, kCritNull);
    msda::begin_call();
    return msda::launch_criterion_fwd(a, p, losses, stats, (hipStream_t)stream);
}

int msda_criterion_bwd_f32(int kind, const float *const *pred_logits, const float *const *pred_hand_key,
                           const float *const *pred_obj_key, int sets, int bs, int Q, int K, int D, const int64_t *match,
                           int t_max, const int64_t *labels, const float *keypoints, const int64_t *offsets,
                           long long n_targets, const int32_t *is_valid, const uint8_t *joint_valid,
                           unsigned long long hand_mask, const float *num_boxes, float focal_alpha,
                           const float *grad_losses, const int32_t *stats, float *const *grad_logits,
                           float *const *grad_hand_key, float *const *grad_obj_key, msda_stream_t stream)
{
    msda::CritArgs a;
    msda::PredSets<const float> p;
    int rc = check_criterion("msda_criterion_bwd_f32", kind, pred_logits, pred_hand_key, pred_obj_key, sets, bs, Q, K, D, match,
                             t_max, labels, keypoints, offsets, n_targets, is_valid, joint_valid, hand_mask, num_boxes,
                             focal_alpha, a, p);
    if (rc != MSDA_OK) return rc;
    if (grad_losses == nullptr || stats == nullptr) return msda::set_error(MSDA_ERR_ARGUMENT, kCritNull);
    const bool has_kp = keypoints != nullptr, arctic = kind == MSDA_CRITERION_ARCTIC;
    msda::PredSets<float> g;
    rc = bind_sets(kCritNull, sets, grad_logits, grad_hand_key, grad_obj_key, has_kp, has_kp && arctic, g);
    if (rc != MSDA_OK) return rc;
    msda::begin_call();
    return msda::launch_criterion_bwd(a, p, g, grad_losses, stats, (hipStream_t)stream);
}

/* ---- the DINO criterion's matched and denoising losses (msda_criterion_dino.hip) ---- */
static const char kDinoCritNull[] = "msda_criterion_dino: null pointer";
static int check_criterion_dino(const char *who, const float *const *pred_logits, const float *const *pred_hand_key,
                                const float *const *pred_obj_key, const int *Q, const int *match_set, int sets, int bs, int K,
                                int D, int single_pad, int groups, const int64_t *match, int match_sets, int t_max,
                                const int64_t *labels, const float *keypoints, const int64_t *offsets, long long n_targets,
                                const int32_t *is_valid, unsigned long long hand_mask, const float *num_boxes,
                                float focal_alpha, msda::DinoCritArgs &a, msda::PredSets<const float> &p)
{
    int rc = check_set_range(who, sets, bs, 1);
    if (rc != MSDA_OK) return rc;
    if (K < 1 || D < 0 || n_targets < 0) return refuse_set(who, "need K >= 1, D >= 0 and n_targets >= 0");
    const bool has_kp = keypoints != nullptr;
    rc = check_target_dim(who, has_kp, D, 0);
    if (rc != MSDA_OK) return rc;
    if (pred_logits == nullptr || Q == nullptr || match_set == nullptr || offsets == nullptr || num_boxes == nullptr
        || is_valid == nullptr || (n_targets > 0 && labels == nullptr)
        || (has_kp && (pred_hand_key == nullptr || pred_obj_key == nullptr)))
        return msda::set_error(MSDA_ERR_ARGUMENT, kDinoCritNull);
    if (targets_beyond_2g(n_targets, D)) return refuse_beyond_2g("msda_criterion_dino");
    p = {};
    a = {};
    long long chunks = 0;
    for (int s = 0; s < sets; ++s) {   // a set's own conditions come before its pointers, so they bind one set at a time
        if (Q[s] < 1) return refuse_set(who, "need Q[s] >= 1 in every set");
        if (match_set[s] < 0) {
            if (groups < 1 || single_pad < 1 || (long long)groups * single_pad != Q[s])
                return refuse_set(who, "a denoising set needs groups >= 1, single_pad >= 1 and Q[s] = groups * single_pad");
        } else {
            if (match_set[s] >= match_sets || t_max < 0 || t_max > msda::kMatchMaxTargets)
                return refuse_set(who, "a matched set needs match_set[s] < match_sets and 0 <= t_max <= %d",
                                  msda::kMatchMaxTargets);
            if (match == nullptr) return msda::set_error(MSDA_ERR_ARGUMENT, "msda_criterion_dino: null pointer (match)");
        }
        if (preds_beyond_2g(bs, Q[s], K, D)) return refuse_beyond_2g("msda_criterion_dino");
        if (!bind_set(s, pred_logits, pred_hand_key, pred_obj_key, has_kp, has_kp, p))
            return msda::set_error(MSDA_ERR_ARGUMENT, kDinoCritNull);
        a.Q[s] = Q[s];
        a.match_set[s] = match_set[s] < 0 ? -1 : match_set[s];
        a.chunk_base[s] = (int)chunks;
        chunks += (long long)bs * ((Q[s] + msda::kDinoCritChunkRows - 1) / msda::kDinoCritChunkRows);   // < 2^31 / 256 * 16
    }
    a.sets = sets;
    a.bs = bs;
    a.K = K;
    a.D = D;
    a.match_sets = match_sets;
    a.single_pad = single_pad;
    a.groups = groups;
    a.match = match;
    a.tg = {labels, keypoints, offsets, n_targets, is_valid, t_max};
    a.hand_mask = hand_mask;
    a.num_boxes = num_boxes;
    a.alpha = focal_alpha;
    a.chunks = (int)chunks;
    return MSDA_OK;
}

int msda_criterion_dino_fwd_f32(const float *const *pred_logits, const float *const *pred_hand_key,
                                const float *const *pred_obj_key, const int *Q, const int *match_set, int sets, int bs, int K,
                                int D, int single_pad, int groups, const int64_t *match, int match_sets, int t_max,
                                const int64_t *labels, const float *keypoints, const int64_t *offsets, long long n_targets,
                                const int32_t *is_valid, unsigned long long hand_mask, const float *num_boxes,
                                float focal_alpha, void *workspace, unsigned long long workspace_bytes, float *losses,
                                int32_t *stats, msda_stream_t stream)
{
    msda::DinoCritArgs a;
    msda::PredSets<const float> p;
    int rc = check_criterion_dino("msda_criterion_dino_fwd_f32", pred_logits, pred_hand_key, pred_obj_key, Q, match_set, sets, bs,
                                  K, D, single_pad, groups, match, match_sets, t_max, labels, keypoints, offsets, n_targets,
                                  is_valid, hand_mask, num_boxes, focal_alpha, a, p);
    if (rc != MSDA_OK) return rc;
    if (losses == nullptr || stats == nullptr || workspace == nullptr) return msda::set_error(MSDA_ERR_ARGUMENT, kDinoCritNull);
    if (((uintptr_t)workspace & 7u) != 0 || workspace_bytes < (unsigned long long)a.chunks * msda::kDinoCritPartialBytes)
        return msda::set_error(MSDA_ERR_ARGUMENT, "msda_criterion_dino_fwd_f32: the workspace needs 8-byte alignment and "
                                                  "MSDA_CRITERION_DINO_PARTIAL_BYTES per chunk");
    msda::begin_call();
    return msda::launch_criterion_dino_fwd(a, p, workspace, losses, stats, (hipStream_t)stream);
}

int msda_criterion_dino_bwd_f32(const float *const *pred_logits, const float *const *pred_hand_key,
                                const float *const *pred_obj_key, const int *Q, const int *match_set, int sets, int bs, int K,
                                int D, int single_pad, int groups, const int64_t *match, int match_sets, int t_max,
                                const int64_t *labels, const float *keypoints, const int64_t *offsets, long long n_targets,
                                const int32_t *is_valid, unsigned long long hand_mask, const float *num_boxes,
                                float focal_alpha, const float *grad_losses, const int32_t *stats, float *const *grad_logits,
                                float *const *grad_hand_key, float *const *grad_obj_key, msda_stream_t stream)
{
    msda::DinoCritArgs a;
    msda::PredSets<const float> p;
    int rc = check_criterion_dino("msda_criterion_dino_bwd_f32", pred_logits, pred_hand_key, pred_obj_key, Q, match_set, sets, bs,
                                  K, D, single_pad, groups, match, match_sets, t_max, labels, keypoints, offsets, n_targets,
                                  is_valid, hand_mask, num_boxes, focal_alpha, a, p);
    if (rc != MSDA_OK) return rc;
    if (grad_losses == nullptr || stats == nullptr) return msda::set_error(MSDA_ERR_ARGUMENT, kDinoCritNull);
    const bool has_kp = keypoints != nullptr;
    msda::PredSets<float> g;
    rc = bind_sets(kDinoCritNull, sets, grad_logits, grad_hand_key, grad_obj_key, has_kp, has_kp, g);
    if (rc != MSDA_OK) return rc;
    msda::begin_call();
    return msda::launch_criterion_dino_bwd(a, p, g, grad_losses, stats, (hipStream_t)stream);
}

/* ---- the DETR prediction heads, fp32 and under bf16 autocast (msda_heads.hip plans both; msda_heads_bf16.hip) ---- */
int msda_heads_supported(int C) { return msda::heads_supported(msda::kHeadsF32, C) ? 1 : 0; }
int msda_heads_bf16_supported(int C) { return msda::heads_supported(msda::kHeadsBf16, C) ? 1 : 0; }

static unsigned long long heads_workspace(int form, int kind, int L, long long M, int C, int K, int n_mlp, unsigned flags)
{
    if (L < 1 || L > msda::kHeadsMaxLevels || M < 1 || C < 1 || K < 1 || n_mlp < 0 || n_mlp > msda::kHeadsMaxMlp) return 0;
    return msda::heads_workspace_bytes(form, kind, L, M, C, K, n_mlp, flags);
}

unsigned long long msda_heads_workspace_bytes(int kind, int L, long long M, int C, int K, int n_mlp, unsigned flags)
{
    return heads_workspace(msda::kHeadsF32, kind, L, M, C, K, n_mlp, flags);
}

unsigned long long msda_heads_bf16_workspace_bytes(int kind, int L, long long M, int C, int K, int n_mlp, unsigned flags)
{
    return heads_workspace(msda::kHeadsBf16, kind, L, M, C, K, n_mlp, flags);
}

/* The operands every entry has; the forward entries add their outputs, the backward entries their gradients and workspace.
 * An entry's typed pointer arrays (float *const *, uint16_t *const *) become the call's void *const *: arrays of addresses. */
static msda::HeadsCall heads_call(int form, int kind, int L, long long M, int C, int K, int n_mlp, int R, unsigned flags,
                                  const float *hs, const float *init_ref, const float *inter_ref, const float *const *cls_w,
                                  const float *const *cls_b, const float *const *mlp_w, const float *const *mlp_b,
                                  const float *const *shared_w, const float *const *shared_b, const void *hidden, const float *sig)
{
    msda::HeadsCall c = {};
    c.form = form; c.kind = kind; c.L = L; c.M = M; c.C = C; c.K = K; c.n_mlp = n_mlp; c.R = R; c.flags = flags;
    c.hs = hs; c.init_ref = init_ref; c.inter_ref = inter_ref;
    c.cls_w = cls_w; c.cls_b = cls_b; c.mlp_w = mlp_w; c.mlp_b = mlp_b; c.shared_w = shared_w; c.shared_b = shared_b;
    c.hidden = const_cast<void *>(hidden); c.sig = const_cast<float *>(sig);
    return c;
}

/* the one plan of each direction that this thread's calls of either form build and launch */
static int heads_forward(msda::HeadsCall &c, void *logits, const void *kp_out, const void *shared_out, msda_stream_t stream)
{
    c.logits = logits; c.kp_out = static_cast<void *const *>(kp_out); c.shared_out = static_cast<void *const *>(shared_out);
    static thread_local msda::HeadsFwdPlan plan;
    const int rc = msda::heads_plan_forward(c, plan);
    if (rc != MSDA_OK) return rc;
    msda::begin_call();
    return msda::heads_run_forward(plan, (hipStream_t)stream);
}

static int heads_backward(msda::HeadsCall &c, const void *grad_logits, const void *grad_kp, const void *grad_shared,
                          float *grad_hs, float *const *grad_cls_w, float *const *grad_cls_b, float *const *grad_mlp_w,
                          float *const *grad_mlp_b, float *const *grad_shared_w, float *const *grad_shared_b, void *workspace,
                          unsigned long long workspace_bytes, msda_stream_t stream)
{
    c.grad_logits = grad_logits; c.grad_kp = static_cast<const void *const *>(grad_kp);
    c.grad_shared = static_cast<const void *const *>(grad_shared); c.grad_hs = grad_hs;
    c.grad_cls_w = grad_cls_w; c.grad_cls_b = grad_cls_b; c.grad_mlp_w = grad_mlp_w; c.grad_mlp_b = grad_mlp_b;
    c.grad_shared_w = grad_shared_w; c.grad_shared_b = grad_shared_b; c.ws = workspace; c.ws_bytes = workspace_bytes;
    static thread_local msda::HeadsBwdPlan plan;
    const int rc = msda::heads_plan_backward(c, plan);
    if (rc != MSDA_OK) return rc;
    msda::begin_call();
    return msda::heads_run_backward(plan, (hipStream_t)stream);
}

int msda_heads_forward_f32(int kind, int L, long long M, int C, int K, int n_mlp, int R, unsigned flags, const float *hs,
                           const float *init_ref, const float *inter_ref, const float *const *cls_w,
                           const float *const *cls_b, const float *const *mlp_w, const float *const *mlp_b,
                           const float *const *shared_w, const float *const *shared_b, float *logits, float *const *kp_out,
                           float *const *shared_out, float *hidden, float *sig, msda_stream_t stream)
{
    msda::HeadsCall c = heads_call(msda::kHeadsF32, kind, L, M, C, K, n_mlp, R, flags, hs, init_ref, inter_ref, cls_w, cls_b,
                                   mlp_w, mlp_b, shared_w, shared_b, hidden, sig);
    return heads_forward(c, logits, kp_out, shared_out, stream);
}

int msda_heads_backward_f32(int kind, int L, long long M, int C, int K, int n_mlp, int R, unsigned flags, const float *hs,
                            const float *init_ref, const float *inter_ref, const float *const *cls_w,
                            const float *const *cls_b, const float *const *mlp_w, const float *const *mlp_b,
                            const float *const *shared_w, const float *const *shared_b, const float *hidden,
                            const float *sig, const float *grad_logits, const float *const *grad_kp,
                            const float *const *grad_shared, float *grad_hs, float *const *grad_cls_w,
                            float *const *grad_cls_b, float *const *grad_mlp_w, float *const *grad_mlp_b,
                            float *const *grad_shared_w, float *const *grad_shared_b, void *workspace,
                            unsigned long long workspace_bytes, msda_stream_t stream)
{
    msda::HeadsCall c = heads_call(msda::kHeadsF32, kind, L, M, C, K, n_mlp, R, flags, hs, init_ref, inter_ref, cls_w, cls_b,
                                   mlp_w, mlp_b, shared_w, shared_b, hidden, sig);
    return heads_backward(c, grad_logits, grad_kp, grad_shared, grad_hs, grad_cls_w, grad_cls_b, grad_mlp_w, grad_mlp_b,
                          grad_shared_w, grad_shared_b, workspace, workspace_bytes, stream);
}

int msda_heads_ref_backward_f32(int L, long long M, int n_mlp, int R, const float *init_ref, const float *inter_ref,
                                const float *sig, const float *const *grad_kp, float *grad_init_ref, float *grad_inter_ref,
                                msda_stream_t stream)
{
    msda::HeadsRefBwdPlan plan;
    const int rc = msda::heads_plan_ref_backward(L, M, n_mlp, R, init_ref, inter_ref, sig, grad_kp, grad_init_ref, grad_inter_ref, plan);
    if (rc != MSDA_OK) return rc;
    msda::begin_call();
    return msda::heads_run_ref_backward(plan, (hipStream_t)stream);
}

int msda_heads_forward_bf16(int kind, int L, long long M, int C, int K, int n_mlp, int R, unsigned flags, const float *hs,
                            const float *init_ref, const float *inter_ref, const float *const *cls_w,
                            const float *const *cls_b, const float *const *mlp_w, const float *const *mlp_b,
                            const float *const *shared_w, const float *const *shared_b, void *logits, void *const *kp_out,
                            uint16_t *const *shared_out, uint16_t *hidden, float *sig, msda_stream_t stream)
{
    msda::HeadsCall c = heads_call(msda::kHeadsBf16, kind, L, M, C, K, n_mlp, R, flags, hs, init_ref, inter_ref, cls_w, cls_b,
                                   mlp_w, mlp_b, shared_w, shared_b, hidden, sig);
    return heads_forward(c, logits, kp_out, shared_out, stream);
}

int msda_heads_backward_bf16(int kind, int L, long long M, int C, int K, int n_mlp, int R, unsigned flags, const float *hs,
                             const float *init_ref, const float *inter_ref, const float *const *cls_w,
                             const float *const *cls_b, const float *const *mlp_w, const float *const *mlp_b,
                             const float *const *shared_w, const float *const *shared_b, const uint16_t *hidden,
                             const float *sig, const void *grad_logits, const void *const *grad_kp,
                             const uint16_t *const *grad_shared, float *grad_hs, float *const *grad_cls_w,
                             float *const *grad_cls_b, float *const *grad_mlp_w, float *const *grad_mlp_b,
                             float *const *grad_shared_w, float *const *grad_shared_b, void *workspace,
                             unsigned long long workspace_bytes, msda_stream_t stream)
{
    msda::HeadsCall c = heads_call(msda::kHeadsBf16, kind, L, M, C, K, n_mlp, R, flags, hs, init_ref, inter_ref, cls_w, cls_b,
                                   mlp_w, mlp_b, shared_w, shared_b, hidden, sig);
    return heads_backward(c, grad_logits, grad_kp, grad_shared, grad_hs, grad_cls_w, grad_cls_b, grad_mlp_w, grad_mlp_b,
                          grad_shared_w, grad_shared_b, workspace, workspace_bytes, stream);
}

/* ---- the layers' FFN under bf16 autocast (msda_ffn_bf16.hip): models/arctic_transformer.py:283-287, :366-370 ---- */
int msda_ffn_bf16_supported(int C, int F) { return msda::ffn_bf16_supported(C, F) ? 1 : 0; }

unsigned long long msda_ffn_bf16_workspace_bytes(long long M, int C, int F) { return msda::ffn_bf16_workspace_bytes(M, C, F); }

int msda_ffn_forward_bf16(long long M, int C, int F, const void *x, int x_is_bf16, const float *w1, const float *b1, const float *w2,
                          const float *b2, double p, const long long *seed, uint16_t *xb, uint16_t *a, uint16_t *y,
                          msda_stream_t stream)
{
    if (int rc = msda::ffn_check_forward_bf16(M, C, F, x, x_is_bf16, w1, b1, w2, b2, p, seed, xb, a, y)) return rc;
    msda::begin_call();
    return msda::launch_ffn_forward_bf16(M, C, F, x, x_is_bf16, w1, b1, w2, b2, p, seed, xb, a, y, (hipStream_t)stream);
}

int msda_ffn_backward_bf16(long long M, int C, int F, const uint16_t *grad_out, const uint16_t *xb, const uint16_t *a, const float *w1,
                           const float *w2, double p, void *grad_x, int grad_x_is_bf16, float *grad_w1, float *grad_b1,
                           float *grad_w2, float *grad_b2, void *workspace, unsigned long long workspace_bytes, msda_stream_t stream)
{
    if (int rc = msda::ffn_check_backward_bf16(M, C, F, grad_out, xb, a, w1, w2, p, grad_x, grad_w1, grad_b1, grad_w2, grad_b2,
                                               workspace, workspace_bytes))
        return rc;
    msda::begin_call();
    return msda::launch_ffn_backward_bf16(M, C, F, grad_out, xb, a, w1, w2, p, grad_x, grad_x_is_bf16, grad_w1, grad_b1, grad_w2,
                                          grad_b2, workspace, (hipStream_t)stream);
}

/* ---- Swin window attention (msda_swin.hip): replaces models/swin_transformer.py:126-142 (WindowAttention.forward's scores,
 * relative position bias, mask, softmax and weighted sum), :210-240 (SwinTransformerBlock's pad, roll, partition, reverse, roll
 * back and crop) and :339-357 (BasicLayer's shift mask) ---- */
int msda_swin_attn_supported(int B, int H, int W, int C, int nH, int ws, int shift)
{
    return msda::swin_supported(B, H, W, C, nH, ws, shift) ? 1 : 0;
}

unsigned long long msda_swin_attn_workspace_bytes(int B, int H, int W, int C, int nH, int ws, int shift, int which)
{
    return msda::swin_workspace_bytes(B, H, W, C, nH, ws, shift, which);
}

int msda_swin_attn_forward_f32(int B, int H, int W, int C, int nH, int ws, int shift, const float *qkv, const float *qkv_bias,
                               const float *table, float *out, float *lse, unsigned long long lse_bytes, msda_stream_t stream)
{
    msda::begin_call();
    return msda::swin_forward(B, H, W, C, nH, ws, shift, qkv, qkv_bias, table, out, lse, lse_bytes, (hipStream_t)stream);
}

int msda_swin_attn_backward_f32(int B, int H, int W, int C, int nH, int ws, int shift, const float *qkv, const float *qkv_bias,
                                const float *table, const float *out, const float *lse, unsigned long long lse_bytes,
                                const float *grad_out, float *grad_qkv, float *grad_table, float *grad_qkv_bias, void *workspace,
                                unsigned long long workspace_bytes, msda_stream_t stream)
{
    msda::begin_call();
    return msda::swin_backward(B, H, W, C, nH, ws, shift, qkv, qkv_bias, table, out, lse, lse_bytes, grad_out, grad_qkv,
                               grad_table, grad_qkv_bias, workspace, workspace_bytes, (hipStream_t)stream);
}

int msda_swin_attn_forward_bf16(int B, int H, int W, int C, int nH, int ws, int shift, const uint16_t *qkv, const float *qkv_bias,
                                const float *table, uint16_t *out, float *lse, unsigned long long lse_bytes, msda_stream_t stream)
{
    msda::begin_call();
    return msda::swin_forward_bf16(B, H, W, C, nH, ws, shift, qkv, qkv_bias, table, out, lse, lse_bytes, (hipStream_t)stream);
}

int msda_swin_attn_backward_bf16(int B, int H, int W, int C, int nH, int ws, int shift, const uint16_t *qkv,
                                 const float *qkv_bias, const float *table, const uint16_t *out, const float *lse,
                                 unsigned long long lse_bytes, const uint16_t *grad_out, uint16_t *grad_qkv, float *grad_table,
                                 float *grad_qkv_bias, void *workspace, unsigned long long workspace_bytes, msda_stream_t stream)
{
    msda::begin_call();
    return msda::swin_backward_bf16(B, H, W, C, nH, ws, shift, qkv, qkv_bias, table, out, lse, lse_bytes, grad_out, grad_qkv,
                                    grad_table, grad_qkv_bias, workspace, workspace_bytes, (hipStream_t)stream);
}

// ---- the Swin blocks' glue (msda_swin_glue.hip): every check is the launcher's, before its first launch ----
int msda_swin_glue_supported(int C) { return msda::swin_glue_supported(C) ? 1 : 0; }

unsigned long long msda_swin_glue_workspace_bytes(long long rows, int C) { return msda::swin_glue_workspace_bytes(rows, C); }

// X: the residual stream's type (x, y and their gradients), T: the branch's and the normalised rows'; SUF <T> or <T>_sbf16
#define MSDA_SWIN_GLUE_NORM_ENTRIES(X, T, SUF, SBF, BF)                                                                          \
    int msda_swin_glue_norm_forward_##SUF(const X *x, const float *gamma, const float *beta, long long rows, int C, float eps,   \
                                          T *z, float *mean, float *rstd, msda_stream_t stream)                                  \
    {                                                                                                                            \
        msda::begin_call();                                                                                                      \
        return msda::swin_glue_norm_forward(SBF, BF, x, gamma, beta, rows, C, eps, z, mean, rstd, (hipStream_t)stream);          \
    }                                                                                                                            \
    int msda_swin_glue_norm_backward_##SUF(const T *grad_z, const X *x, const float *gamma, const float *mean,                   \
                                           const float *rstd, long long rows, int C, X *grad_x, float *grad_gamma,               \
                                           float *grad_beta, void *workspace, unsigned long long workspace_bytes,                \
                                           msda_stream_t stream)                                                                 \
    {                                                                                                                            \
        msda::begin_call();                                                                                                      \
        return msda::swin_glue_norm_backward(SBF, BF, grad_z, x, gamma, mean, rstd, rows, C, grad_x, grad_gamma, grad_beta,      \
                                             workspace, workspace_bytes, (hipStream_t)stream);                                   \
    }
#define MSDA_SWIN_GLUE_ENTRIES(X, T, SUF, SBF, BF)                                                                               \
    MSDA_SWIN_GLUE_NORM_ENTRIES(X, T, SUF, SBF, BF)                                                                              \
    int msda_swin_glue_add_norm_forward_##SUF(const X *x, const T *a, const T *keep, long long rows,                             \
                                              long long rows_per_sample, int C, const float *gamma, const float *beta,           \
                                              float eps, X *y, T *z, float *mean, float *rstd, msda_stream_t stream)             \
    {                                                                                                                            \
        msda::begin_call();                                                                                                      \
        return msda::swin_glue_add_norm_forward(SBF, BF, x, a, keep, rows, rows_per_sample, C, gamma, beta, eps, y, z, mean,     \
                                                rstd, (hipStream_t)stream);                                                      \
    }                                                                                                                            \
    int msda_swin_glue_add_norm_backward_##SUF(const X *grad_y, const T *grad_z, const X *y, const T *keep,                      \
                                               const float *gamma, const float *mean, const float *rstd, long long rows,         \
                                               long long rows_per_sample, int C, X *grad_x, T *grad_a, float *grad_gamma,        \
                                               float *grad_beta, void *workspace, unsigned long long workspace_bytes,            \
                                               msda_stream_t stream)                                                             \
    {                                                                                                                            \
        msda::begin_call();                                                                                                      \
        return msda::swin_glue_add_norm_backward(SBF, BF, grad_y, grad_z, y, keep, gamma, mean, rstd, rows, rows_per_sample, C,  \
                                                 grad_x, grad_a, grad_gamma, grad_beta, workspace, workspace_bytes,              \
                                                 (hipStream_t)stream);                                                           \
    }                                                                                                                            \
    int msda_swin_glue_add_forward_##SUF(const X *x, const T *a, const T *keep, long long rows, long long rows_per_sample,       \
                                         int C, X *y, msda_stream_t stream)                                                      \
    {                                                                                                                            \
        msda::begin_call();                                                                                                      \
        return msda::swin_glue_add_forward(SBF, BF, x, a, keep, rows, rows_per_sample, C, y, (hipStream_t)stream);               \
    }                                                                                                                            \
    int msda_swin_glue_add_backward_##SUF(const X *grad_y, const T *keep, long long rows, long long rows_per_sample, int C,      \
                                          T *grad_a, msda_stream_t stream)                                                       \
    {                                                                                                                            \
        msda::begin_call();                                                                                                      \
        return msda::swin_glue_add_backward(SBF, BF, grad_y, keep, rows, rows_per_sample, C, grad_a, (hipStream_t)stream);       \
    }                                                                                                                            \
    int msda_swin_glue_merge_norm_forward_##SUF(const X *x, int B, int H, int W, int C, const float *gamma,                      \
                                                const float *beta, float eps, T *z, float *mean, float *rstd,                    \
                                                msda_stream_t stream)                                                            \
    {                                                                                                                            \
        msda::begin_call();                                                                                                      \
        return msda::swin_glue_merge_norm_forward(SBF, BF, x, B, H, W, C, gamma, beta, eps, z, mean, rstd,                       \
                                                  (hipStream_t)stream);                                                          \
    }                                                                                                                            \
    int msda_swin_glue_merge_norm_backward_##SUF(const T *grad_z, const X *x, const float *gamma, const float *mean,             \
                                                 const float *rstd, int B, int H, int W, int C, X *grad_x,                       \
                                                 float *grad_gamma, float *grad_beta, void *workspace,                           \
                                                 unsigned long long workspace_bytes, msda_stream_t stream)                       \
    {                                                                                                                            \
        msda::begin_call();                                                                                                      \
        return msda::swin_glue_merge_norm_backward(SBF, BF, grad_z, x, gamma, mean, rstd, B, H, W, C, grad_x, grad_gamma,        \
                                                   grad_beta, workspace, workspace_bytes, (hipStream_t)stream);                  \
    }
MSDA_SWIN_GLUE_ENTRIES(float, float, f32, false, false)
MSDA_SWIN_GLUE_ENTRIES(float, uint16_t, bf16, false, true)
MSDA_SWIN_GLUE_ENTRIES(uint16_t, uint16_t, bf16_sbf16, true, true)
MSDA_SWIN_GLUE_NORM_ENTRIES(uint16_t, float, f32_sbf16, true, false)       // the per-stage output norms of a bf16 stream
#undef MSDA_SWIN_GLUE_ENTRIES
#undef MSDA_SWIN_GLUE_NORM_ENTRIES

// ---- the tail of the step (msda_optim.hip): engine.py:644-648's clip_grad_norm_ and optimizer.step(), util/settings.py:434's
// AdamW and util/misc.py's get_total_grad_norm; every check is the launcher's, before its launch ----
int msda_optim_supported(long long n_tensors, int n_groups) { return msda::optim_supported(n_tensors, n_groups) ? 1 : 0; }

int msda_optim_chunk_elems(void) { return msda::kOptimChunk; }

long long msda_optim_chunks(int n_tensors, const long long *numel, long long *chunk_start)
{
    return msda::optim_chunks(n_tensors, numel, chunk_start);
}

int msda_grad_sumsq_f32(int n_tensors, long long n_chunks, const float *const *g, const long long *numel,
                        const long long *chunk_start, float *partials, msda_stream_t stream)
{
    msda::begin_call();
    return msda::launch_grad_sumsq(n_tensors, n_chunks, g, numel, chunk_start, partials, (hipStream_t)stream);
}

int msda_grad_norm_finish_f32(long long n_chunks, const float *partials, float max_norm, float *out, msda_stream_t stream)
{
    msda::begin_call();
    return msda::launch_grad_norm_finish(n_chunks, partials, max_norm, out, (hipStream_t)stream);
}

int msda_grad_scale_f32(int n_tensors, long long n_chunks, float *const *g, const long long *numel, const long long *chunk_start,
                        const float *coef, msda_stream_t stream)
{
    msda::begin_call();
    return msda::launch_grad_scale(n_tensors, n_chunks, g, numel, chunk_start, coef, (hipStream_t)stream);
}

int msda_adamw_step_f32(int n_tensors, long long n_chunks, float *const *p, const float *const *g, float *const *exp_avg,
                        float *const *exp_avg_sq, const long long *numel, const long long *chunk_start, const int *group,
                        const long long *step_offset, int n_groups, const double *lr, const double *weight_decay,
                        const double *beta1, const double *beta2, const double *eps, long long global_step, const float *coef,
                        msda_stream_t stream)
{
    msda::begin_call();
    msda::OptimTables t;
    t.n = n_tensors; t.n_chunks = n_chunks; t.p = p; t.g = g; t.exp_avg = exp_avg; t.exp_avg_sq = exp_avg_sq;
    t.numel = numel; t.chunk_start = chunk_start; t.group = group; t.step_offset = step_offset;
    return msda::launch_adamw_step(t, n_groups, lr, weight_decay, beta1, beta2, eps, global_step, coef, (hipStream_t)stream);
}

// the device-state forms of the same tail (engine.py:644-648, util/settings.py:434-440): steps and hyperparameters live on the device
int msda_optim_advance_f32(int n_tensors, float *const *step, msda_stream_t stream)
{
    msda::begin_call();
    return msda::launch_optim_advance(n_tensors, step, (hipStream_t)stream);
}

int msda_grad_norm_finish_dev_f32(long long n_chunks, const float *partials, float max_norm, float *out, int n_tensors,
                                  float *const *step, int skip_nonfinite, int *status, msda_stream_t stream)
{
    msda::begin_call();
    return msda::launch_grad_norm_finish_dev(n_chunks, partials, max_norm, out, n_tensors, step, skip_nonfinite, status,
                                             (hipStream_t)stream);
}

int msda_adamw_step_dev_f32(int n_tensors, long long n_chunks, float *const *p, const float *const *g, float *const *exp_avg,
                            float *const *exp_avg_sq, const long long *numel, const long long *chunk_start, const int *group,
                            const float *const *step, int n_groups, const double *hyper, const float *coef, const int *skip,
                            msda_stream_t stream)
{
    msda::begin_call();
    msda::OptimTables t;
    t.n = n_tensors; t.n_chunks = n_chunks; t.p = p; t.g = g; t.exp_avg = exp_avg; t.exp_avg_sq = exp_avg_sq;
    t.numel = numel; t.chunk_start = chunk_start; t.group = group; t.step_offset = nullptr;
    return msda::launch_adamw_step_dev(t, step, n_groups, hyper, coef, skip, (hipStream_t)stream);
}

}  // extern "C"
