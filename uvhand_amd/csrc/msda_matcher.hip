// The Hungarian matchers (UVHand models/matcher.py: ArcticMatcher :20-125, AssemblyMatcher :128-230) in one launch: one
// workgroup per (prediction set, output frame slot) builds that frame's cost block on chip and solves its assignment, so
// the batch-wide [bs*Q, sum T] matrix, its copy to the host and the per-frame scipy call are gone.
//
//   cost block  one thread per query q of output frame k, T <= 16 targets (the chunk of the k-th VALID frame: the
//               reference splits the valid frames' targets by their sizes and pairs chunk k with output frame k, :122-123,
//               which differs from the chunk's own frame when an earlier frame is invalid; is_valid == NULL: chunk k is
//               frame k).  In the reference's fp32 order (no contraction):
//                 p = sigmoid(logit[lab]), neg = (0.75 p^2) (-log(1 - p + 1e-8)), pos = (0.25 (1-p)^2) (-log(p + 1e-8)),
//                 C = w_kp * L1 + w_cls * (pos - neg)      (C = w_cls * (pos - neg) when there are no target keypoints)
//               L1 over D values against the hand head for labels 12 / 13, 0 for label 0, the object head otherwise
//               (:76-119); the Assembly entry passes its one keypoint head as both, which is :191-224 (L1 where label != 0).
//   solve       scipy's rectangular LSAP (the shortest augmenting path of Crouse 2016, fp64 duals over the fp32 costs) on
//               the nr x nc problem nr = min(Q, T) <= 16 rows, nc = max(Q, T) <= 1024 columns, transposed as scipy
//               transposes a tall matrix: targets are the rows when T < Q.  One thread per column holds that column's
//               nr costs, its dual, shortest-path cost and path in registers; the rows' duals and assignment live in LDS.
//               Each Dijkstra step is one argmin over the remaining columns (wave64 butterfly, then the waves' results in
//               LDS) with scipy's exact tie rule: among equal minima an unassigned column wins, the last one in scipy's
//               `remaining` order, else the first; the `remaining` array's swap-remove order is tracked per column.  The
//               fp64 arithmetic is scipy's expression by expression, so the result is scipy's, ties included.
//   status      0, 1 = a NaN or -inf cost (scipy: "matrix contains invalid numeric entries"), 2 = no finite full
//               assignment ("cost matrix is infeasible"), 3 = a label outside [0, K), 4 = offsets that do not describe
//               the targets.  The kernel never traps.
//
// Output (int64, one buffer): query_idx [sets, bs, W], target_idx [sets, bs, W] (query indices ascending, -1 padding),
// count [sets, bs] (min(Q, T); -1 for slots past the number of valid frames), status [sets, bs], then (matcher only) the
// number of valid frames.
#include <math.h>

#include "msda_common.h"
#include "msda_launch.h"

#pragma clang fp contract(off)

namespace msda {

namespace {

constexpr int kMtRows = kMatchMaxTargets;          // rows of the solved problem (min(Q, T))
constexpr int kMtWaves = kMatchMaxQueries / 64;     // waves of the widest workgroup
constexpr int kMtAbsent = -1;                       // tie key of a column that is not a candidate
constexpr int kMtUnassigned = 2048;                 // tie key offset of an unassigned column (above any assigned one)

struct MtCand {
    double val;     // shortest-path cost
    int tb;         // tie key: unassigned -> 2048 + pos (last in scan order wins), assigned -> 1023 - pos (first wins)
    int j;          // column
    int path;       // its predecessor row
    int r4c;        // its row, -1 if unassigned
};

struct MtShared {
    MtCand red[2][kMtWaves];                 // per-wave argmins, double-buffered across steps
    double u[kMtRows];                       // row duals
    int col4row[kMtRows];
    int step_j[kMtRows + 1], step_path[kMtRows + 1];   // columns picked by the current augmentation, in order
    int chain_j[kMtRows + 1], chain_i[kMtRows + 1], chain_n;
    float stage[kMtRows * kMtRows];          // a wide block (Q <= T) handed from query threads to target threads
    int lab[kMtRows];
    float kp[kMtRows * kMatchMaxDim];
    int wcnt[kMtWaves];
    int frame, lo, T, status;
};

__device__ __forceinline__ bool mt_better(const MtCand &a, const MtCand &b)
{
    return a.val < b.val || (a.val == b.val && a.tb > b.tb);
}

__device__ __forceinline__ MtCand mt_shfl(const MtCand &c, int m)
{
    MtCand o;
    o.val = __shfl_xor(c.val, m, 64);
    o.tb = __shfl_xor(c.tb, m, 64);
    o.j = __shfl_xor(c.j, m, 64);
    o.path = __shfl_xor(c.path, m, 64);
    o.r4c = __shfl_xor(c.r4c, m, 64);
    return o;
}

// A column's costs: a register vector.  Its runtime index i is block-uniform; made scalar it selects a VGPR
// (v_movrels), where a plain array indexed at run time is moved to LDS or scratch.
typedef float MtCol __attribute__((ext_vector_type(kMtRows)));

__device__ __forceinline__ float mt_pick(const MtCol &col, int i) { return col[__builtin_amdgcn_readfirstlane(i)]; }

// Solves the nr x nc problem (1 <= nr <= 16, nr <= nc <= blockDim.x) whose column j = threadIdx.x has the costs
// col[0..nr-1]; every thread of the block calls it.  Returns 0 with sh.col4row[0..nr-1] = each row's column, or
// kMatchInfeasible.  scipy's solve() / augmenting_path() (rectangular_lsap.cpp) step by step.
__device__ int mt_solve(int nr, int nc, const MtCol &col, MtShared &sh)
{
    const int j = threadIdx.x, lane = j & 63, w = j >> 6, nw = blockDim.x >> 6;
    const bool act = j < nc;
    const double inf = (double)INFINITY;
    double v = 0.0;
    int r4c = -1;
    if (j < nr) { sh.u[j] = 0.0; sh.col4row[j] = -1; }
    __syncthreads();
    int par = 0;
    for (int cur = 0; cur < nr; ++cur) {
        double spc = inf, min_val = 0.0;
        int pth = -1, pos = nc - 1 - j, nrem = nc, i = cur, nsteps = 0, sink = -1;
        bool sc = false;
        while (true) {
            const double ui = sh.u[i];
            if (act && !sc) {
                const double r = min_val + (double)mt_pick(col, i) - ui - v;
                if (r < spc) { spc = r; pth = i; }
            }
            MtCand c;
            if (act && !sc) c = MtCand{spc, r4c < 0 ? kMtUnassigned + pos : 1023 - pos, j, pth, r4c};
            else c = MtCand{inf, kMtAbsent, -1, -1, -1};
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
                const MtCand o = mt_shfl(c, m);
                if (mt_better(o, c)) c = o;
            }
            if (lane == 0) sh.red[par][w] = c;
            __syncthreads();
            MtCand best = sh.red[par][0];
            for (int x = 1; x < nw; ++x) {
                const MtCand o = sh.red[par][x];
                if (mt_better(o, best)) best = o;
            }
            par ^= 1;
            if (best.val == inf || best.tb == kMtAbsent) return kMatchInfeasible;   // block-uniform
            min_val = best.val;
            const int winpos = best.tb >= kMtUnassigned ? best.tb - kMtUnassigned : 1023 - best.tb;
            if (j == best.j) sc = true;
            else if (act && !sc && pos == nrem - 1) pos = winpos;   // remaining[index] = remaining[--num_remaining]
            --nrem;
            if (j == 0 && nsteps <= kMtRows) { sh.step_j[nsteps] = best.j; sh.step_path[nsteps] = best.path; }
            ++nsteps;
            if (best.r4c < 0) { sink = best.j; break; }
            if (best.r4c >= nr || nsteps > nr) return kMatchInfeasible;   // unreachable; keeps every LDS index in range
            i = best.r4c;
        }
        // duals: every thread has read sh.u for the last step (before the last barrier)
        if (act && sc) {
            if (r4c >= 0) sh.u[r4c] += min_val - spc;
            v -= min_val - spc;
        }
        if (j == 0) sh.u[cur] += min_val;
        __syncthreads();
        if (j == 0) {   // augment along the path from the sink back to row cur
            int jj = sink, n = 0;
            while (n <= nr) {
                int ii = -1;
                for (int s = 0; s < nsteps && s <= kMtRows; ++s)
                    if (sh.step_j[s] == jj) ii = sh.step_path[s];
                if (ii < 0 || ii >= nr) break;
                sh.chain_j[n] = jj;
                sh.chain_i[n] = ii;
                ++n;
                const int old = sh.col4row[ii];
                sh.col4row[ii] = jj;
                jj = old;
                if (ii == cur) break;
            }
            sh.chain_n = n;
        }
        __syncthreads();
        for (int s = 0; s < sh.chain_n; ++s)
            if (sh.chain_j[s] == j) r4c = sh.chain_i[s];
    }
    return 0;
}

// Solves the block (T < Q: targets are the rows; else queries are) and writes slot `slot` of the output: pairs sorted by
// query index, -1 padding to W, count, status.  col = this thread's column as mt_solve wants it.
__device__ void mt_finish(int Q, int T, const MtCol &col, int status, MtShared &sh, int64_t *out, const MatchView &mv,
                          long long slot)
{
    const int W = mv.W;
    const int nr = T < Q ? T : Q;
    const int nc = T < Q ? Q : T;
    if (status == 0 && nr > 0) status = mt_solve(nr, nc, col, sh);
    __syncthreads();
    const int count = status == 0 ? nr : 0;
    int64_t *qo = out + mv.query(slot, 0);
    int64_t *to = out + mv.target(slot, 0);
    const int t = threadIdx.x;
    if (t < W) {
        if (t >= count) {
            qo[t] = -1;
            to[t] = -1;
        } else if (T < Q) {   // row t = target t, matched to query col4row[t]: its rank among the matched queries
            const int q = sh.col4row[t];
            int rank = 0;
            for (int x = 0; x < nr; ++x) rank += sh.col4row[x] < q;
            qo[rank] = q;
            to[rank] = t;
        } else {              // row t = query t
            qo[t] = t;
            to[t] = sh.col4row[t];
        }
    }
    if (t == 0) {
        out[mv.count(slot)] = count;
        out[mv.status(slot)] = status;
    }
}

__device__ __forceinline__ bool mt_bad(float c) { return c != c || c == -INFINITY; }

__global__ __launch_bounds__(kMatchMaxQueries) void match_kernel(PredSets<const float> sets, int bs, int Q, int K, int D,
                                                                 const int64_t *__restrict__ labels,
                                                                 const float *__restrict__ tgt_kp,
                                                                 const int64_t *__restrict__ offsets, long long n_targets,
                                                                 const int32_t *__restrict__ is_valid, int t_max, float w_cls,
                                                                 float w_kp, int64_t *__restrict__ out,
                                                                 float *__restrict__ cost_debug)
{
    __shared__ MtShared sh;
    const int k = blockIdx.x, s = blockIdx.y;
    const MatchView mv(gridDim.y, bs, t_max);
    const long long slot = (long long)s * bs + k;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, nw = blockDim.x >> 6;

    // the frame whose targets go with output slot k: the k-th valid frame (a prefix over is_valid)
    int nvalid = bs;
    if (tid == 0) sh.frame = is_valid ? -1 : k;
    __syncthreads();
    if (is_valid) {
        int base = 0;
        for (int f0 = 0; f0 < bs; f0 += blockDim.x) {
            const int f = f0 + tid;
            const bool valid = f < bs && is_valid[f] != 0;
            const unsigned long long b = __ballot(valid);
            const int rank = __popcll(b & ((1ull << lane) - 1ull));
            if (lane == 0) sh.wcnt[w] = __popcll(b);
            __syncthreads();
            int before = 0, total = 0;
            for (int x = 0; x < nw; ++x) {
                before += x < w ? sh.wcnt[x] : 0;
                total += sh.wcnt[x];
            }
            if (valid && base + before + rank == k) sh.frame = f;
            base += total;
            __syncthreads();
        }
        nvalid = base;
    }
    if (slot == 0 && tid == 0) out[mv.nvalid()] = nvalid;

    if (tid == 0) {
        int status = 0, T = 0;
        long long lo = 0;
        const int f = sh.frame;
        if (f >= 0) {
            lo = offsets[f];
            const long long hi = offsets[f + 1];
            if (lo < 0 || hi < lo || hi > n_targets || hi - lo > t_max) status = kMatchBadTargets;
            else T = (int)(hi - lo);
        }
        sh.lo = (int)lo;
        sh.T = T;
        sh.status = status;
    }
    __syncthreads();
    if (sh.frame < 0) {   // past the valid frames: no chunk pairs with this slot
        if (tid < t_max) {
            out[mv.query(slot, tid)] = -1;
            out[mv.target(slot, tid)] = -1;
        }
        if (tid == 0) {
            out[mv.count(slot)] = -1;
            out[mv.status(slot)] = 0;
        }
        return;
    }
    const int T = sh.T;
    const long long lo = sh.lo;
    if (sh.status == 0) {
        if (tid < T) {
            const long long lab = labels[lo + tid];
            sh.lab[tid] = (int)lab;
            if (lab < 0 || lab >= K) sh.status = kMatchBadLabel;
        }
        if (tgt_kp)
            for (int x = tid; x < T * D; x += blockDim.x) sh.kp[x] = tgt_kp[lo * D + x];
    }
    __syncthreads();
    int status = sh.status;

    MtCol col = 0.f;
    bool bad = false;
    if (status == 0 && tid < Q) {
        const long long row = (long long)k * Q + tid;
        const float *lg = sets.logits[s] + row * K;
        const float *hk = tgt_kp ? sets.hand[s] + row * D : nullptr;
        const float *ok = tgt_kp ? sets.obj[s] + row * D : nullptr;
#pragma unroll
        for (int t = 0; t < kMtRows; ++t) {
            if (t < T) {
                const int lab = sh.lab[t];
                const float p = 1.f / (1.f + expf(-lg[lab]));
                const float neg = (0.75f * (p * p)) * (-logf((1.f - p) + 1e-8f));
                const float pos = (0.25f * ((1.f - p) * (1.f - p))) * (-logf(p + 1e-8f));
                const float cls = pos - neg;
                float c;
                if (tgt_kp) {
                    float l1 = 0.f;
                    if (lab != 0) {
                        const float *src = (lab == 12 || lab == 13) ? hk : ok;
                        const float *tk = sh.kp + t * D;
                        for (int d = 0; d < D; ++d) l1 += fabsf(src[d] - tk[d]);
                    }
                    c = w_kp * l1 + w_cls * cls;
                } else {
                    c = w_cls * cls;
                }
                col[t] = c;
                bad |= mt_bad(c);
                if (cost_debug) cost_debug[(slot * Q + tid) * t_max + t] = c;
            }
        }
    }
    if (__syncthreads_or(bad) && status == 0) status = kMatchInvalid;
    if (status == 0 && T >= Q && T > 0) {   // wide block: queries are the rows, the target threads take the columns
        if (tid < Q)
#pragma unroll
            for (int t = 0; t < kMtRows; ++t)
                if (t < T) sh.stage[tid * kMtRows + t] = col[t];
        __syncthreads();
#pragma unroll
        for (int i = 0; i < kMtRows; ++i) col[i] = (tid < T && i < Q) ? sh.stage[i * kMtRows + tid] : 0.f;
    }
    mt_finish(Q, T, col, status, sh, out, mv, slot);
}

__global__ __launch_bounds__(kMatchMaxQueries) void lsap_kernel(const float *__restrict__ cost, int Q, int T, int W, long long B,
                                                                int64_t *__restrict__ out)
{
    __shared__ MtShared sh;
    const long long b = blockIdx.x;
    const int j = threadIdx.x;
    const float *c = cost + b * Q * T;
    MtCol col;
    bool bad = false;
#pragma unroll
    for (int i = 0; i < kMtRows; ++i) {
        float x = 0.f;
        if (T < Q) {              // column j = query j, rows = targets
            if (j < Q && i < T) x = c[(long long)j * T + i];
        } else {                  // column j = target j, rows = queries
            if (j < T && i < Q) x = c[(long long)i * T + j];
        }
        bad |= mt_bad(x);
        col[i] = x;
    }
    const int status = __syncthreads_or(bad) ? kMatchInvalid : 0;
    mt_finish(Q, T, col, status, sh, out, MatchView(B, 1, W), b);   // B one-frame sets, no valid-frame count
}

}  // namespace

int launch_match(const PredSets<const float> &sets, int n_sets, int bs, int Q, int K, int D, const SetTargets &tg, float w_cls,
                 float w_kp, int64_t *out, float *cost_debug, hipStream_t stream)
{
    if (bs == 0) return MSDA_OK;
    const int threads = ((Q > kMtRows ? Q : kMtRows) + 63) / 64 * 64;
    // the kernel takes the targets member by member: its pointers are __restrict__, which a record's members cannot be
    hipLaunchKernelGGL(match_kernel, dim3((unsigned)bs, (unsigned)n_sets), dim3(threads), 0, stream, sets, bs, Q, K, D, tg.labels,
                       tg.tgt_kp, tg.offsets, tg.n_targets, tg.is_valid, tg.t_max, w_cls, w_kp, out, cost_debug);
    return check_launch("match_kernel");
}

int launch_lsap(const float *cost, int B, int Q, int T, int64_t *out, hipStream_t stream)
{
    if (B == 0) return MSDA_OK;
    const int wide = Q > T ? Q : T;
    const int threads = (wide + 63) / 64 * 64;
    hipLaunchKernelGGL(lsap_kernel, dim3((unsigned)B), dim3(threads), 0, stream, cost, Q, T, Q < T ? Q : T, (long long)B, out);
    return check_launch("lsap_kernel");
}

}  // namespace msda
