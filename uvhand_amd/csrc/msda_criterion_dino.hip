// The matched and denoising losses of DINO's criterion (models/dino/dino.py SetCriterion: loss_labels / loss_cardinality /
// loss_boxes :453-532, the denoising losses :615-664) for every prediction set of a step in one forward pass (two launches)
// and one backward launch, with nothing read on the host.  The sets may differ in query count: the final, aux and interm sets
// have num_queries rows per frame and take their pairs from the matcher's device result (msda_matcher.hip); a denoising set
// has groups * single_pad rows and its pairs are fixed (:623-633), so no match buffer is read for it.
//
//   pairing    slot k pairs output frame k with the k-th VALID frame f's targets (the reference's chunk pairing).  A matched
//              set reads slot k of its set in `match`; a denoising set pairs query g * single_pad + j with target
//              offsets[f] + j for every g < groups, j < n_f.  n_f > single_pad / 2 (prepare_for_cdn never makes it) sets the
//              bad-targets bit and the frame gives no pair.
//   forward    a chunk is up to 256 rows of one (set, output frame).  One workgroup per chunk: one thread per row finds the
//              row's positive, then the focal loss over the chunk's logits and the L1 over its positive keypoint rows element
//              by element (coalesced), per-thread fp64 partials summed in a fixed order, the argmax count and the hand /
//              object row counts as integers; the chunk's record goes to the caller's workspace.  A second launch, one
//              workgroup per set, adds the records (each thread a fixed stride of them, then the fixed-order block sum) and
//              writes `losses` and `stats`.  No workgroup waits for another; no float atomics: bitwise reproducible, and a
//              set's result does not depend on the other sets of the call.
//                loss_ce      focal(alpha, gamma 2).mean(1).sum() / num_boxes * Q   (denoising: / (num_boxes * groups))
//                keypoints    hand head L1 over positive rows with labels in hand_mask / their count / 21 (0 without one),
//                             object head over the other positive rows / their count / 21 (0 / 0 = nan, as the reference)
//                cardinality  mean over frames f of |#(argmax of output frame f's rows != K - 1) - n_f|
//              every term is 0 when no valid frame has a target.
//   backward   one workgroup per chunk: the positives again, then every logit's focal derivative and every keypoint
//              element's sign(src - tgt) * scale (zero off the positive rows), coalesced.  Every element is written.
//   status     per set, bits as msda_criterion.hip: 1 a paired label outside [0, K), 2 offsets or target indices that do not
//              describe the targets (or n_f > single_pad / 2), 8 a matcher slot status.  The kernels never trap.
#include <math.h>

#include "msda_common.h"
#include "msda_criterion_common.h"
#include "msda_launch.h"

#pragma clang fp contract(off)

namespace msda {

namespace {

constexpr int kDcThreads = kDinoCritChunkRows;
constexpr int kDcWaves = kDcThreads / 64;

struct DcPartial {
    double ce, hand, obj;
    int status, n_hand, n_obj, card;   // card: rows of the chunk whose argmax is not the empty class
    int pad[6];
};
static_assert(sizeof(DcPartial) == kDinoCritPartialBytes, "include/msda.h documents the record size");

struct DcChunk {
    int s, k, q0, nr, c;   // set, output frame, first row, rows, index within the frame
    bool dn;
};

__device__ __forceinline__ DcChunk dc_chunk(const DinoCritArgs &a, int chunk)
{
    DcChunk ch;
    ch.s = 0;
    for (int i = 1; i < a.sets; ++i)
        if (chunk >= a.chunk_base[i]) ch.s = i;
    const int Q = a.Q[ch.s], cpf = (Q + kDinoCritChunkRows - 1) / kDinoCritChunkRows;
    const int local = chunk - a.chunk_base[ch.s];
    ch.k = local / cpf;
    ch.c = local % cpf;
    ch.q0 = ch.c * kDinoCritChunkRows;
    ch.nr = Q - ch.q0 < kDinoCritChunkRows ? Q - ch.q0 : kDinoCritChunkRows;
    ch.dn = a.match_set[ch.s] < 0;
    return ch;
}

// The positive of row q of slot k of set s: true with its label and target row; status bits are or-ed into st.
__device__ bool dc_positive(const DinoCritArgs &a, const DcChunk &ch, int q, const int *frame_of, int &label, long long &trow,
                            int &st)
{
    const int f = frame_of[ch.k];
    if (f < 0) return false;   // past the valid frames
    long long lo, hi, j = -1;
    if (!cr_frame_targets(a.tg, f, lo, hi)) {
        st |= kCritBadTargets;
        return false;
    }
    const long long n = hi - lo;
    if (ch.dn) {
        if (n > a.single_pad / 2) {
            st |= kCritBadTargets;
            return false;
        }
        j = q % a.single_pad;
        if (j >= n) return false;
    } else {
        const MatchView mv(a.match_sets, a.bs, a.tg.t_max);
        const long long slot = (long long)a.match_set[ch.s] * a.bs + ch.k;
        const long long cnt = a.match[mv.count(slot)];
        int m = 0;
        for (; m < cnt && m < mv.W; ++m) {   // pairs are in ascending query order
            const long long qm = a.match[mv.query(slot, m)];
            if (qm == q) break;
            if (qm > q) return false;
        }
        if (!(m < cnt && m < mv.W)) return false;
        j = a.match[mv.target(slot, m)];
        if (j < 0 || j >= n || m >= n) {
            st |= kCritBadTargets;
            return false;
        }
    }
    const long long lab = a.tg.labels[lo + j];
    if (lab < 0 || lab >= a.K) {
        st |= kCritBadLabel;
        return false;
    }
    label = (int)lab;
    trow = lo + j;
    return true;
}

// What no row of the slot can notice: the matcher's slot status and pairs whose query lies outside the set.
__device__ int dc_slot_status(const DinoCritArgs &a, const DcChunk &ch, const int *frame_of)
{
    const int tid = threadIdx.x, f = frame_of[ch.k];
    int st = 0;
    long long lo = 0, hi = 0;
    const bool ok = f >= 0 && cr_frame_targets(a.tg, f, lo, hi);
    if (tid == 0 && f >= 0 && !ok) st |= kCritBadTargets;
    if (ch.dn) {
        if (tid == 0 && ok && hi - lo > a.single_pad / 2) st |= kCritBadTargets;
        return st;
    }
    const MatchView mv(a.match_sets, a.bs, a.tg.t_max);
    const long long slot = (long long)a.match_set[ch.s] * a.bs + ch.k;
    if (tid == 0 && a.match[mv.status(slot)] != 0) st |= kCritMatchStatus;
    const long long cnt = a.match[mv.count(slot)];
    if (tid < mv.W && tid < cnt) {
        const long long q = a.match[mv.query(slot, tid)];
        if (!ok || q < 0 || q >= a.Q[ch.s]) st |= kCritBadTargets;
    }
    return st;
}

struct DcShared {
    int frame_of[kMatchMaxQueries];   // slot -> frame whose targets pair with it (-1 past the valid frames)
    int wcnt[kDcWaves];
    int lab[kDcThreads];              // the chunk's rows: positive label or -1
    long long trow[kDcThreads];       // and target row or -1
    double dred[3][kDcWaves];
    int ints[4];                      // status bits, hand rows, object rows, non-empty rows
};

__global__ __launch_bounds__(kDcThreads) void criterion_dino_chunk_kernel(DinoCritArgs a, PredSets<const float> p,
                                                                          DcPartial *__restrict__ part)
{
    __shared__ DcShared sh;
    const int tid = threadIdx.x;
    const DcChunk ch = dc_chunk(a, blockIdx.x);
    const int K = a.K, D = a.D, Q = a.Q[ch.s];
    cr_slot_frames(a.tg.is_valid, a.bs, sh.frame_of, sh.wcnt);
    if (tid < 4) sh.ints[tid] = 0;
    __syncthreads();

    const long long r0 = (long long)ch.k * Q + ch.q0;
    const float *x = p.logits[ch.s] + r0 * K;
    int status = ch.c == 0 ? dc_slot_status(a, ch, sh.frame_of) : 0, n_hand = 0, n_obj = 0, n_full = 0;
    if (tid < ch.nr) {
        int label = -1;
        long long trow = -1;
        if (dc_positive(a, ch, ch.q0 + tid, sh.frame_of, label, trow, status)) {
            const bool hand = cr_hand(a.hand_mask, label);
            n_hand += hand;
            n_obj += !hand;
        }
        sh.lab[tid] = label;
        sh.trow[tid] = trow;
        n_full = cr_argmax(x + (long long)tid * K, K) != K - 1;
    }
    __syncthreads();

    double csum = 0.0, hsum = 0.0, osum = 0.0;
    for (int i = tid; i < ch.nr * K; i += kDcThreads) {
        const int rl = i / K, c = i % K;
        csum += (double)cr_focal(x[i], c == sh.lab[rl] ? 1.f : 0.f, a.alpha);
    }
    if (a.tg.tgt_kp) {
        const float *ph = p.hand[ch.s] + r0 * D, *po = p.obj[ch.s] + r0 * D;
        for (int i = tid; i < ch.nr * D; i += kDcThreads) {
            const int rl = i / D, d = i % D;
            const long long tr = sh.trow[rl];
            if (tr < 0) continue;
            const float t = a.tg.tgt_kp[tr * D + d];
            if (cr_hand(a.hand_mask, sh.lab[rl])) hsum += (double)fabsf(ph[i] - t);
            else osum += (double)fabsf(po[i] - t);
        }
    }
    if (status) atomicOr(&sh.ints[0], status);   // integers: order-free
    if (n_hand) atomicAdd(&sh.ints[1], n_hand);
    if (n_obj) atomicAdd(&sh.ints[2], n_obj);
    if (n_full) atomicAdd(&sh.ints[3], n_full);
    csum = cr_block_sum(csum, sh.dred[0]);
    hsum = cr_block_sum(hsum, sh.dred[1]);
    osum = cr_block_sum(osum, sh.dred[2]);   // its barrier also orders the LDS integers
    if (tid == 0) {
        DcPartial out = {};
        out.ce = csum;
        out.hand = hsum;
        out.obj = osum;
        out.status = sh.ints[0];
        out.n_hand = sh.ints[1];
        out.n_obj = sh.ints[2];
        out.card = sh.ints[3];
        part[blockIdx.x] = out;
    }
}

__global__ __launch_bounds__(kDcThreads) void criterion_dino_finish_kernel(DinoCritArgs a, const DcPartial *__restrict__ part,
                                                                           float *__restrict__ losses,
                                                                           int32_t *__restrict__ stats)
{
    __shared__ double dred[3][kDcWaves];
    __shared__ int ints[5];   // status bits, hand rows, object rows, |card error|, valid frames with a target
    const int s = blockIdx.x, tid = threadIdx.x;
    const int bs = a.bs, Q = a.Q[s], cpf = (Q + kDinoCritChunkRows - 1) / kDinoCritChunkRows;
    const bool dn = a.match_set[s] < 0;
    const DcPartial *mine = part + a.chunk_base[s];
    if (tid < 5) ints[tid] = 0;
    __syncthreads();

    int status = 0, n_hand = 0, n_obj = 0, card_err = 0, valid_targets = 0;
    double csum = 0.0, hsum = 0.0, osum = 0.0;
    for (int i = tid; i < bs * cpf; i += kDcThreads) {   // a fixed stride per thread: the order depends on the sizes alone
        const DcPartial r = mine[i];
        csum += r.ce;
        hsum += r.hand;
        osum += r.obj;
        status |= r.status;
        n_hand += r.n_hand;
        n_obj += r.n_obj;
    }
    for (int f = tid; f < bs; f += kDcThreads) {
        int full = 0;
        for (int c = 0; c < cpf; ++c) full += mine[f * cpf + c].card;
        long long lo, hi;
        const bool ok = cr_frame_targets(a.tg, f, lo, hi);
        const long long d = full - (hi - lo);
        card_err += (int)(d < 0 ? -d : d);
        if (a.tg.is_valid[f] != 0) {
            if (!ok) status |= kCritBadTargets;
            else valid_targets += (int)(hi - lo > 0);
        }
    }
    if (status) atomicOr(&ints[0], status);   // integers: order-free
    atomicAdd(&ints[1], n_hand);
    atomicAdd(&ints[2], n_obj);
    atomicAdd(&ints[3], card_err);
    atomicAdd(&ints[4], valid_targets);
    csum = cr_block_sum(csum, dred[0]);
    hsum = cr_block_sum(hsum, dred[1]);
    osum = cr_block_sum(osum, dred[2]);   // its barrier also orders the LDS integers
    if (tid == 0) {
        n_hand = ints[1];
        n_obj = ints[2];
        const float nb = dn ? *a.num_boxes * (float)a.groups : *a.num_boxes;
        const bool none = ints[4] == 0;   // the reference's matcher has nothing to match: every term is 0
        float *out = losses + (long long)s * kCritTerms;
        out[0] = none ? 0.f : (float)(csum / (double)Q / (double)nb * (double)Q);
        out[1] = (none || n_hand == 0) ? 0.f : ((float)hsum / (float)n_hand) / 21.f;
        out[2] = none ? 0.f : (n_obj == 0 ? NAN : ((float)osum / (float)n_obj) / 21.f);
        out[3] = none ? 0.f : (float)ints[3] / (float)bs;
        int32_t *st = stats + (long long)s * kCritStats;
        st[0] = ints[0];
        st[1] = n_hand;
        st[2] = n_obj;
        st[3] = none ? 1 : 0;
    }
}

__global__ __launch_bounds__(kDcThreads) void criterion_dino_bwd_kernel(DinoCritArgs a, PredSets<const float> p,
                                                                        PredSets<float> g,
                                                                        const float *__restrict__ grad_losses,
                                                                        const int32_t *__restrict__ stats)
{
    __shared__ int frame_of[kMatchMaxQueries];
    __shared__ int wcnt[kDcWaves];
    __shared__ int lab[kDcThreads];
    __shared__ long long trow[kDcThreads];
    const int tid = threadIdx.x;
    const DcChunk ch = dc_chunk(a, blockIdx.x);
    const int K = a.K, D = a.D, Q = a.Q[ch.s];
    cr_slot_frames(a.tg.is_valid, a.bs, frame_of, wcnt);
    __syncthreads();

    const int32_t *st = stats + (long long)ch.s * kCritStats;
    const bool none = st[3] != 0;
    const int n_hand = st[1], n_obj = st[2];
    const float *gl = grad_losses + (long long)ch.s * kCritTerms;
    const float nb = ch.dn ? *a.num_boxes * (float)a.groups : *a.num_boxes;
    const float ce_scale = none ? 0.f : ((gl[0] * (float)Q) / nb) / (float)Q;   // torch: * Q, / num_boxes, mean over Q
    const float h_scale = (none || n_hand == 0) ? 0.f : (gl[1] / 21.f) / (float)n_hand;
    const float o_scale = (none || n_obj == 0) ? 0.f : (gl[2] / 21.f) / (float)n_obj;

    if (tid < ch.nr) {
        int label = -1, ignored = 0;
        long long tr = -1;
        dc_positive(a, ch, ch.q0 + tid, frame_of, label, tr, ignored);
        lab[tid] = label;
        trow[tid] = tr;
    }
    __syncthreads();

    const long long r0 = (long long)ch.k * Q + ch.q0;
    const float *x = p.logits[ch.s] + r0 * K;
    float *gx = g.logits[ch.s] + r0 * K;
    for (int i = tid; i < ch.nr * K; i += kDcThreads) {
        const int rl = i / K, c = i % K;
        gx[i] = ce_scale * cr_focal_grad(x[i], c == lab[rl], a.alpha);
    }
    if (D == 0) return;
    float *gh = g.hand[ch.s] + r0 * D, *go = g.obj[ch.s] + r0 * D;
    const float *ph = p.hand[ch.s] + r0 * D, *po = p.obj[ch.s] + r0 * D;
    for (int i = tid; i < ch.nr * D; i += kDcThreads) {
        const int rl = i / D, d = i % D;
        const long long tr = trow[rl];
        float vh = 0.f, vo = 0.f;
        if (tr >= 0) {
            const float t = a.tg.tgt_kp[tr * D + d];
            if (cr_hand(a.hand_mask, lab[rl])) {
                const float diff = ph[i] - t;
                vh = h_scale * (float)((diff > 0.f) - (diff < 0.f));
            } else {
                const float diff = po[i] - t;
                vo = o_scale * (float)((diff > 0.f) - (diff < 0.f));
            }
        }
        gh[i] = vh;
        go[i] = vo;
    }
}

}  // namespace

int launch_criterion_dino_fwd(const DinoCritArgs &a, const PredSets<const float> &p, void *workspace, float *losses,
                              int32_t *stats, hipStream_t stream)
{
    DcPartial *part = static_cast<DcPartial *>(workspace);
    hipLaunchKernelGGL(criterion_dino_chunk_kernel, dim3((unsigned)a.chunks), dim3(kDcThreads), 0, stream, a, p, part);
    int rc = check_launch("criterion_dino_chunk_kernel");
    if (rc != MSDA_OK) return rc;
    hipLaunchKernelGGL(criterion_dino_finish_kernel, dim3((unsigned)a.sets), dim3(kDcThreads), 0, stream, a, part, losses, stats);
    return check_launch("criterion_dino_finish_kernel");
}

int launch_criterion_dino_bwd(const DinoCritArgs &a, const PredSets<const float> &p, const PredSets<float> &g,
                              const float *grad_losses, const int32_t *stats, hipStream_t stream)
{
    hipLaunchKernelGGL(criterion_dino_bwd_kernel, dim3((unsigned)a.chunks), dim3(kDcThreads), 0, stream, a, p, g, grad_losses, stats);
    return check_launch("criterion_dino_bwd_kernel");
}

}  // namespace msda
