// One call of the sampling op as its host layer passes it on: the geometry, the call's tensors and its options.  The C entries
// (msda_abi.hip) fill these records, the launchers and planners of both kernel families (msda_d32.hip, msda_generic.hip) read them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "msda.h"

namespace msda {

inline int pow2_shift(int x) { return (x > 0 && (x & (x - 1)) == 0) ? __builtin_ctz((unsigned)x) : -1; }

struct OpGeom {
    int N, S, M, D, L, Lq, P;
    bool nonempty() const { return N > 0 && S > 0 && M > 0 && D > 0 && L > 0 && Lq > 0 && P > 0; }
    long long items() const { return (long long)N * Lq * M; }          // (batch, query, head) triples
    int LP() const { return L * P; }
    int p_shift() const { return pow2_shift(P); }                       // log2, or -1 where not a power of two
    int lp_shift() const { return pow2_shift(L * P); }
    int m_shift() const { return pow2_shift(M); }
};

// loc, attn and their gradients: fp32 beside fp32 and bf16 rows, fp64 beside fp64 rows
template <typename VT> using op_real_t = std::conditional_t<sizeof(VT) == 8, double, float>;

// VT = storage of value / out / grad_out: float, double, or uint16_t (bf16 bits).  The plain entries leave the fused
// prologue's part empty; with it, loc / attn are the raw offsets / logits and ld_* the floats between their (batch, query) rows.
template <typename VT>
struct FwdTensors {
    const VT *value;
    const int64_t *shapes, *level_start;
    const op_real_t<VT> *loc, *attn;
    VT *out;
    hipStream_t stream;
    const float *ref;                     // fused prologue: reference points [N, Lq, L, 2]
    float *loc_out, *attn_out;            // ... the sampling locations and attention weights it leaves for the backward
    long long ld_offsets, ld_logits;
};

// GT = storage of grad_value: VT, or float beside bf16 rows.  With the fused prologue grad_loc / grad_attn are the gradients of
// the raw offsets / logits, with rows ld_* floats apart.
template <typename VT, typename GT>
struct BwdTensors {
    const VT *grad_out, *value;
    const int64_t *shapes, *level_start;
    const op_real_t<VT> *loc, *attn;
    GT *grad_value;
    op_real_t<VT> *grad_loc, *grad_attn;
    hipStream_t stream;
    float *grad_ref;                      // fused prologue: [N, Lq, L, 2]
    long long ld_grad_offsets, ld_grad_logits;
};

// The caller's workspace (forward: room for the table; backward: that table first, the call's scratch behind it) and the
// MSDA_FLAG_* bits of the call.
struct OpOptions {
    void *workspace;
    size_t ws_bytes;
    bool deterministic, forward_table, exact_nonfinite;
    OpOptions(void *ws = nullptr, unsigned long long bytes = 0, unsigned flags = 0)
        : workspace(ws), ws_bytes((size_t)bytes), deterministic((flags & MSDA_FLAG_DETERMINISTIC) != 0),
          forward_table((flags & MSDA_FLAG_FORWARD_TABLE) != 0), exact_nonfinite((flags & MSDA_FLAG_EXACT_NONFINITE) != 0) {}
};

}  // namespace msda
