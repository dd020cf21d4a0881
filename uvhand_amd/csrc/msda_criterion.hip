// The matched losses of UVHand's set criteria (models/actic_detr.py SetArcticCriterion :365-569, models/assembly_detr.py
// SetAssemblyCriterion :248-446) over the device result of the matcher (msda_matcher.hip), every prediction set in one launch
// forward and one launch backward, with no count read on the host.
//
//   match      the matcher's int64 buffer: query_idx [sets, bs, W] (ascending), target_idx [sets, bs, W], count [sets, bs]
//              (-1 past the valid frames), status [sets, bs].  Slot k pairs output frame k with the k-th VALID frame's
//              targets (ARCTIC, a prefix over is_valid, the reference's chunk pairing) or with frame k (AssemblyHands).
//   forward    one workgroup per set, reductions in a fixed order (per-thread fp64 partials, a wave64 butterfly, the
//              waves' partials summed in order by one thread; integer counts through LDS), so results are bitwise
//              reproducible.  Per set:
//                loss_ce    sigmoid focal loss (alpha, gamma 2) of every logit against the one-hot of the matched label
//                           (an unmatched query's row is all zero), .mean(1).sum() / num_boxes * Q
//                keypoints  ARCTIC: sum |hand head - target| over matched hand rows (labels in hand_mask) / their count / 21,
//                           the object head over the other matched rows / their count / 21 (0 / 0 = nan, as the
//                           reference); AssemblyHands: the hand rows' sum where joint_valid / 21, joint_valid row r of a
//                           frame going with the frame's r-th matched row (query order)
//                cardinality  mean over frames of |#(argmax != empty class) - targets of the frame| (ARCTIC: every
//                           frame's targets, invalid frames included; empty class 0, AssemblyHands K - 1)
//                class_error  100 - top-1 accuracy of the matched queries (100 without targets), AssemblyHands
//   backward   one thread per (set, frame, query) row in phase A (its matched target, if any), then the row block's logit
//              and keypoint gradients element by element (coalesced): the focal loss derivative for every logit, sign(src -
//              tgt) times the term's scale on matched keypoint rows, zero elsewhere.  No reduction, no atomics.
//   status     per set, bits: 1 a matched label outside [0, K), 2 offsets or target indices that do not describe the
//              targets, 4 (AssemblyHands) a matched label outside hand_mask or a frame with unmatched targets (the
//              reference's joint_valid mask then mismatches and raises; loss_hand_keypoint is nan), 8 a matcher slot
//              status.  The kernels never trap.
#include <math.h>

#include "msda_common.h"
#include "msda_criterion_common.h"
#include "msda_launch.h"

#pragma clang fp contract(off)

namespace msda {

namespace {

constexpr int kCrFwdThreads = 1024;
constexpr int kCrBwdRows = 256;     // rows (and threads) of a backward workgroup
constexpr int kCrWaves = kCrFwdThreads / 64;

struct CrShared {
    int frame_of[kMatchMaxQueries];   // slot -> frame whose targets pair with it (-1 past the valid frames)
    int card[kMatchMaxQueries];       // forward: non-empty argmax per output frame
    int wcnt[kCrWaves];
    double dred[3][kCrWaves];
    int ints[7];                      // status bits, hand rows, object rows, matched rows, correct, |card error|, valid targets
};

struct CrEntry {
    int q;          // query
    long long row;  // target row (into labels / keypoints)
    int label;
    int m;          // position among the slot's matched pairs
};

// Matched pair m of slot k of set s: 0 and the entry, or a status bit (no pair: -1).
__device__ int cr_entry(const CritArgs &a, int s, int k, int m, const int *frame_of, CrEntry &e)
{
    const MatchView mv(a.sets, a.bs, a.tg.t_max);
    const long long slot = (long long)s * a.bs + k;
    const long long cnt = a.match[mv.count(slot)];
    if (m >= cnt) return -1;
    const long long q = a.match[mv.query(slot, m)], j = a.match[mv.target(slot, m)];
    const int f = frame_of[k];
    if (f < 0) return kCritBadTargets;
    long long lo, hi;
    if (!cr_frame_targets(a.tg, f, lo, hi) || j < 0 || j >= hi - lo || m >= hi - lo || q < 0 || q >= a.Q)
        return kCritBadTargets;
    const long long lab = a.tg.labels[lo + j];
    if (lab < 0 || lab >= a.K) return kCritBadLabel;
    e.q = (int)q;
    e.row = lo + j;
    e.label = (int)lab;
    e.m = m;
    return 0;
}

// The matched pair of row q of slot k, if any (pairs are in ascending query order).
__device__ bool cr_row_entry(const CritArgs &a, int s, int k, int q, const int *frame_of, CrEntry &e)
{
    const MatchView mv(a.sets, a.bs, a.tg.t_max);
    const long long slot = (long long)s * a.bs + k;
    const long long cnt = a.match[mv.count(slot)];
    for (int m = 0; m < cnt && m < mv.W; ++m) {
        const long long qm = a.match[mv.query(slot, m)];
        if (qm == q) return cr_entry(a, s, k, m, frame_of, e) == 0;
        if (qm > q) break;
    }
    return false;
}

__global__ __launch_bounds__(kCrFwdThreads) void criterion_fwd_kernel(CritArgs a, PredSets<const float> p,
                                                                     float *__restrict__ losses, int32_t *__restrict__ stats)
{
    __shared__ CrShared sh;
    const int s = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const int bs = a.bs, Q = a.Q, K = a.K, D = a.D, W = a.tg.t_max;
    const bool assembly = a.kind == kCritAssembly;
    cr_slot_frames(a.tg.is_valid, bs, sh.frame_of, sh.wcnt);
    for (int k = tid; k < bs; k += nt) sh.card[k] = 0;
    if (tid < 7) sh.ints[tid] = 0;
    __syncthreads();

    int status = 0, n_hand = 0, n_obj = 0, n_matched = 0, correct = 0, valid_targets = 0;
    // per slot: matcher status, AssemblyHands' fully matched frames, ARCTIC's valid targets
    const MatchView mv(a.sets, bs, W);
    for (int k = tid; k < bs; k += nt) {
        const long long slot = (long long)s * bs + k;
        if (a.match[mv.status(slot)] != 0) status |= kCritMatchStatus;
        const int f = sh.frame_of[k];
        if (f >= 0) {
            long long lo, hi;
            if (!cr_frame_targets(a.tg, f, lo, hi)) {
                status |= kCritBadTargets;
            } else {
                valid_targets += (int)(hi - lo > 0);
                if (assembly && a.match[mv.count(slot)] != hi - lo) status |= kCritMaskMismatch;
            }
        }
    }
    // matched pairs: hand / object rows, accuracy
    for (int e = tid; e < bs * W; e += nt) {
        CrEntry en;
        const int rc = cr_entry(a, s, e / W, e % W, sh.frame_of, en);
        if (rc > 0) status |= rc;
        if (rc != 0) continue;
        const bool hand = cr_hand(a.hand_mask, en.label);
        n_hand += hand;
        n_obj += !hand;
        if (assembly && !hand) status |= kCritMaskMismatch;
        ++n_matched;
        correct += cr_argmax(p.logits[s] + ((long long)(e / W) * Q + en.q) * K, K) == en.label;
    }
    // keypoint L1 sums over the matched rows
    double hsum = 0.0, osum = 0.0, csum = 0.0;
    if (a.tg.tgt_kp) {
        for (long long i = tid; i < (long long)bs * W * D; i += nt) {
            const int e = (int)(i / D), d = (int)(i % D), k = e / W;
            CrEntry en;
            if (cr_entry(a, s, k, e % W, sh.frame_of, en) != 0) continue;
            const bool hand = cr_hand(a.hand_mask, en.label);
            const long long src = ((long long)k * Q + en.q) * D + d;
            const float t = a.tg.tgt_kp[en.row * D + d];
            if (assembly) {
                const long long jrow = a.tg.offsets[k] + en.m;   // the frame's en.m-th joint_valid row
                if (hand && a.joint_valid[jrow * D + d]) hsum += (double)fabsf(p.hand[s][src] - t);
            } else if (hand) {
                hsum += (double)fabsf(p.hand[s][src] - t);
            } else {
                osum += (double)fabsf(p.obj[s][src] - t);
            }
        }
    }
    // every logit: focal loss; every row: argmax for the cardinality
    const int empty = assembly ? K - 1 : 0;
    for (long long r = tid; r < (long long)bs * Q; r += nt) {
        const int k = (int)(r / Q), q = (int)(r % Q);
        CrEntry en;
        const int lab = cr_row_entry(a, s, k, q, sh.frame_of, en) ? en.label : -1;
        const float *x = p.logits[s] + r * K;
        double rs = 0.0;
        int best = 0;
        float bv = x[0];
        for (int c = 0; c < K; ++c) {
            const float v = x[c];
            rs += (double)cr_focal(v, c == lab ? 1.f : 0.f, a.alpha);
            if (c > 0 && (v > bv || (v != v && bv == bv))) { bv = v; best = c; }
        }
        csum += rs;
        if (best != empty) atomicAdd(&sh.card[k], 1);   // integer: order-free
    }
    __syncthreads();
    int card_err = 0;
    for (int f = tid; f < bs; f += nt) {
        const long long n = a.tg.offsets[f + 1] - a.tg.offsets[f];
        const long long d = sh.card[f] - n;
        card_err += (int)(d < 0 ? -d : d);
    }

    if (status) atomicOr(&sh.ints[0], status);   // integers: order-free
    atomicAdd(&sh.ints[1], n_hand);
    atomicAdd(&sh.ints[2], n_obj);
    atomicAdd(&sh.ints[3], n_matched);
    atomicAdd(&sh.ints[4], correct);
    atomicAdd(&sh.ints[5], card_err);
    atomicAdd(&sh.ints[6], valid_targets);
    csum = cr_block_sum(csum, sh.dred[0]);
    hsum = cr_block_sum(hsum, sh.dred[1]);
    osum = cr_block_sum(osum, sh.dred[2]);   // its barrier also orders the LDS integers
    const int bits = sh.ints[0];
    n_hand = sh.ints[1];
    n_obj = sh.ints[2];
    n_matched = sh.ints[3];
    correct = sh.ints[4];
    card_err = sh.ints[5];
    valid_targets = sh.ints[6];

    if (tid == 0) {
        const float nb = *a.num_boxes;
        const bool none = !assembly && valid_targets == 0;   // the reference's matcher returns 0: every term is 0
        const float ce = none ? 0.f : (float)(csum / (double)Q / (double)nb * (double)Q);
        const float card = none ? 0.f : (float)card_err / (float)bs;
        float *out = losses + (long long)s * kCritTerms;
        if (assembly) {
            const float cls = n_matched == 0 ? 100.f : 100.f - (float)correct * (float)(100.0 / (double)n_matched);
            out[0] = ce;
            out[1] = (bits & kCritMaskMismatch) ? NAN : (float)hsum / 21.f;
            out[2] = card;
            out[3] = cls;
        } else {
            out[0] = ce;
            out[1] = (none || n_hand == 0) ? 0.f : ((float)hsum / (float)n_hand) / 21.f;
            out[2] = none ? 0.f : (n_obj == 0 ? NAN : ((float)osum / (float)n_obj) / 21.f);
            out[3] = card;
        }
        int32_t *st = stats + (long long)s * kCritStats;
        st[0] = bits;
        st[1] = n_hand;
        st[2] = n_obj;
        st[3] = none ? 1 : 0;
    }
}

__global__ __launch_bounds__(kCrBwdRows) void criterion_bwd_kernel(CritArgs a, PredSets<const float> p, PredSets<float> g,
                                                                   const float *__restrict__ grad_losses,
                                                                   const int32_t *__restrict__ stats)
{
    __shared__ int frame_of[kMatchMaxQueries];
    __shared__ int wcnt[kCrBwdRows / 64];
    __shared__ int lab[kCrBwdRows];
    __shared__ long long trow[kCrBwdRows];
    __shared__ int jrow_m[kCrBwdRows];
    const int s = blockIdx.y, tid = threadIdx.x;
    const int bs = a.bs, Q = a.Q, K = a.K, D = a.D;
    const bool assembly = a.kind == kCritAssembly;
    const long long rows = (long long)bs * Q, r0 = (long long)blockIdx.x * kCrBwdRows;
    const int nr = (int)(rows - r0 < kCrBwdRows ? rows - r0 : kCrBwdRows);
    cr_slot_frames(a.tg.is_valid, bs, frame_of, wcnt);
    __syncthreads();

    const int32_t *st = stats + (long long)s * kCritStats;
    const bool none = st[3] != 0, mismatch = (st[0] & kCritMaskMismatch) != 0;
    const int n_hand = st[1], n_obj = st[2];
    const float *gl = grad_losses + (long long)s * kCritTerms;
    const float nb = *a.num_boxes;
    const float ce_scale = none ? 0.f : ((gl[0] * (float)Q) / nb) / (float)Q;   // torch: * Q, / num_boxes, mean over Q
    float h_scale, o_scale = 0.f;
    if (assembly) {
        h_scale = mismatch ? 0.f : gl[1] / 21.f;
    } else {
        h_scale = (none || n_hand == 0) ? 0.f : (gl[1] / 21.f) / (float)n_hand;
        o_scale = (none || n_obj == 0) ? 0.f : (gl[2] / 21.f) / (float)n_obj;
    }

    if (tid < nr) {
        const long long r = r0 + tid;
        CrEntry en;
        const bool m = cr_row_entry(a, s, (int)(r / Q), (int)(r % Q), frame_of, en);
        lab[tid] = m ? en.label : -1;
        trow[tid] = m ? en.row : -1;
        jrow_m[tid] = m ? en.m : -1;
    }
    __syncthreads();

    const float *x = p.logits[s] + r0 * K;
    float *gx = g.logits[s] + r0 * K;
    for (int i = tid; i < nr * K; i += kCrBwdRows) {
        const int rl = i / K, c = i % K;
        gx[i] = ce_scale * cr_focal_grad(x[i], c == lab[rl], a.alpha);
    }
    if (D == 0) return;
    float *gh = g.hand[s] + r0 * D;
    float *go = assembly ? nullptr : g.obj[s] + r0 * D;
    const float *ph = p.hand[s] + r0 * D;
    const float *po = assembly ? nullptr : p.obj[s] + r0 * D;
    for (int i = tid; i < nr * D; i += kCrBwdRows) {
        const int rl = i / D, d = i % D;
        const long long tr = trow[rl];
        float vh = 0.f, vo = 0.f;
        if (tr >= 0 && a.tg.tgt_kp) {
            const float t = a.tg.tgt_kp[tr * D + d];
            const bool hand = cr_hand(a.hand_mask, lab[rl]);
            if (assembly) {
                if (hand && !mismatch) {
                    const int k = (int)((r0 + rl) / Q);
                    const float diff = ph[i] - t;
                    const float sg = (float)((diff > 0.f) - (diff < 0.f));
                    vh = a.joint_valid[(a.tg.offsets[k] + jrow_m[rl]) * D + d] ? h_scale * sg : 0.f;
                }
            } else if (hand) {
                const float diff = ph[i] - t;
                vh = h_scale * (float)((diff > 0.f) - (diff < 0.f));
            } else {
                const float diff = po[i] - t;
                vo = o_scale * (float)((diff > 0.f) - (diff < 0.f));
            }
        }
        gh[i] = vh;
        if (go) go[i] = vo;
    }
}

}  // namespace

int launch_criterion_fwd(const CritArgs &a, const PredSets<const float> &p, float *losses, int32_t *stats,
                         hipStream_t stream)
{
    hipLaunchKernelGGL(criterion_fwd_kernel, dim3((unsigned)a.sets), dim3(kCrFwdThreads), 0, stream, a, p, losses, stats);
    return check_launch("criterion_fwd_kernel");
}

int launch_criterion_bwd(const CritArgs &a, const PredSets<const float> &p, const PredSets<float> &g,
                         const float *grad_losses, const int32_t *stats, hipStream_t stream)
{
    const long long rows = (long long)a.bs * a.Q;
    if (rows == 0) return MSDA_OK;
    const unsigned blocks = (unsigned)((rows + kCrBwdRows - 1) / kCrBwdRows);
    hipLaunchKernelGGL(criterion_bwd_kernel, dim3(blocks, (unsigned)a.sets), dim3(kCrBwdRows), 0, stream, a, p, g, grad_losses,
                       stats);
    return check_launch("criterion_bwd_kernel");
}

}  // namespace msda
