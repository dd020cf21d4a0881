// The one argument record and the one host planner of the four head_dim-32 decoder self-attention cores: resident fp32 and
// bf16 (msda_attn.hip: a (batch, head) pair's operands sit in LDS, lengths up to kAtMaxLen) and streaming fp32 and bf16
// (msda_attn_long.hip: the other operand streams through LDS, lengths up to kAxMaxLen, optional mask).  T is the element type
// of q, k, v, out, dO and the gradients: float, or uint16_t for bf16 bits.  Each of the eight C entries does four things:
// attn_check, attn_bind_forward / attn_bind_backward, size its grid and LDS, launch.  Every refusal is decided here, before
// any launch, with one message per condition that begins with the entry's name.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <initializer_list>

#include "msda_launch.h"

namespace msda {

template <class T>
struct AttnView { T *p; long long sn, sl; };            // element (n, h, l, d) at p + n*sn + h*32 + l*sl + d (strides in elements)

template <class T>
struct AttnArgs {
    AttnView<T> q, k, v, o, go, gq, gk, gv;
    float *lse;                         // [N*H][Lq]
    const unsigned long long *seed;     // device; null when thresh == 0
    const unsigned char *mask;          // streaming cores: [Lq][Lk] bytes, row stride mask_sq; null: none (resident: always)
    long long mask_sq;
    int H, Lq, Lk, wpp;                 // wpp: workgroups per (batch, head) pair
    float scale, scale2, keep_scale;    // scale2 = scale * log2(e): scores are kept in base 2; keep_scale = 1 / (1 - p)
    unsigned thresh;                    // keep iff hash >= thresh (p * 2^32; 0: no dropout)
};

template <class T>
AttnView<T> attn_view(const T *p, long long sn, long long sl) { return AttnView<T>{const_cast<T *>(p), sn, sl}; }

inline int attn_refuse(const char *who, const char *what)
{
    char buf[200];
    snprintf(buf, sizeof(buf), "%s: %s", who, what);
    return set_error(MSDA_ERR_ARGUMENT, buf);
}

// Every check of the geometry, the dropout, the mask and the grid — no view is looked at — and the derived fields.
// max_len: the family's bound (kAtMaxLen, kAxMaxLen); wpp: the most workgroups a launch of the entry gives a pair.
template <class T>
int attn_check(AttnArgs<T> &a, const char *who, int max_len, int N, int H, int Lq, int Lk, int wpp, float scale, float dropout_p,
               const unsigned long long *seed, const unsigned char *mask, long long mask_sq)
{
    char buf[96];
    if (N < 1 || H < 1) return attn_refuse(who, "N >= 1 and H >= 1 required");
    if (Lq < 1 || Lk < 1 || Lq > max_len || Lk > max_len) {
        snprintf(buf, sizeof(buf), "head_dim 32, 1 <= Lq, Lk <= %d", max_len);
        return attn_refuse(who, buf);
    }
    if (!(dropout_p >= 0.f && dropout_p < 1.f)) return attn_refuse(who, "dropout needs 0 <= p < 1");
    if (dropout_p > 0.f && seed == nullptr) return attn_refuse(who, "a device seed is required for p > 0");
    if (mask != nullptr && mask_sq < Lk) return attn_refuse(who, "mask row stride mask_sq must be at least Lk");
    if ((long long)N * H > 0x7fffffffLL / wpp)
        return attn_refuse(who, "too many (batch, head) pairs: N * H * workgroups per pair exceeds 2^31 - 1");
    a.H = H; a.Lq = Lq; a.Lk = Lk; a.wpp = wpp; a.scale = scale;
    a.scale2 = scale * 1.4426950408889634f;
    a.keep_scale = 1.f / (1.f - dropout_p);
    a.thresh = dropout_p > 0.f ? (unsigned)fmin(4294967295.0, (double)dropout_p * 4294967296.0) : 0u;
    a.seed = seed;
    a.mask = mask; a.mask_sq = mask_sq;
    return MSDA_OK;
}

// 16-byte base, strides multiples of 16 bytes: every row is read and written in 16-byte pieces
template <class T>
bool attn_view_ok(const AttnView<T> &v)
{
    constexpr long long m = 16 / sizeof(T) - 1;
    return v.p != nullptr && ((uintptr_t)v.p & 15) == 0 && (v.sn & m) == 0 && (v.sl & m) == 0;
}

template <class T>
int attn_views_ok(const char *who, std::initializer_list<const AttnView<T> *> views, const float *lse)
{
    char buf[96];
    snprintf(buf, sizeof(buf), "16-byte aligned tensors, strides multiples of %d elements", (int)(16 / sizeof(T)));
    for (const AttnView<T> *w : views)
        if (!attn_view_ok(*w)) return attn_refuse(who, buf);
    return lse != nullptr ? MSDA_OK : attn_refuse(who, "lse required");
}

template <class T>
int attn_bind_forward(AttnArgs<T> &a, const char *who, AttnView<T> q, AttnView<T> k, AttnView<T> v, AttnView<T> out, float *lse)
{
    a.q = q; a.k = k; a.v = v; a.o = out; a.lse = lse;
    return attn_views_ok<T>(who, {&a.q, &a.k, &a.v, &a.o}, lse);
}

template <class T>
int attn_bind_backward(AttnArgs<T> &a, const char *who, AttnView<T> q, AttnView<T> k, AttnView<T> v, AttnView<T> out, const float *lse,
                       AttnView<T> grad_out, AttnView<T> grad_q, AttnView<T> grad_k, AttnView<T> grad_v)
{
    a.q = q; a.k = k; a.v = v; a.o = out; a.go = grad_out; a.gq = grad_q; a.gk = grad_k; a.gv = grad_v;
    a.lse = const_cast<float *>(lse);
    return attn_views_ok<T>(who, {&a.q, &a.k, &a.v, &a.o, &a.go, &a.gq, &a.gk, &a.gv}, lse);
}

}  // namespace msda
