// DINO's contrastive-denoising queries (models/dino/dn_components.py:20-150, prepare_for_cdn) and the gradient of the label
// embedding they are read from:
//
//   prepare fwd  ONE launch writes every element of input_query_label [B, pad, H], input_query_key [B, pad, W] and
//                noised_labels [B, pad] (pad = 2 * single_pad * groups).  Row (b, r * single_pad + j) with j < n_b holds target
//                t = offsets[b] + j in repetition r (:67-70 repeat the targets 2 * groups times; :119-123 scatter repetition r of
//                frame b's j-th target to row single_pad * r + j; even r is positive_idx, odd r negative_idx, :82-85): the row
//                of the embedding weight the (possibly replaced, :74-78) label selects, inverse_sigmoid (util/misc.py:614-618)
//                of the keypoints, and the label itself.  Rows with j >= n_b are the reference's zero padding (:111-115), label
//                -1.  A row whose offsets or label do not address the tables (never the case for what the host checked; a
//                replayed graph reads buffers it cannot check) is written as padding: nothing is read out of bounds.
//   draws        the library's counter hash (at_mix / at_hash, msda_attn_tile.h), not torch's stream: flat element
//                e = r * T + t (the reference's order after repeat().view(-1), :67-68), base = at_mix(seed, 0);
//                label replaced iff at_hash(base + 2e) < thr, by (at_hash(base + 2e + 1) * num_classes) >> 32.
//                key noise (key_noise_scale > 0; the reference computes it at :94-103 and drops it, :104-105 being commented
//                out): column c of element e has counters k = 2E + 2 (e W + c), E = 2 * groups * T;
//                sign = bit 31 of at_hash(base + k) ? +1 : -1, u = (at_hash(base + k + 1) >> 8) * 2^-24,
//                part = (u + (r odd ? 1 : 0)) * sign, key' = clamp(key + (part * key) * scale, 0, 1) with every product and sum
//                rounded to nearest on its own (contraction off): the torch restatement gives the same bits.
//   prepare bwd  ONE launch: grad_weight[c] = sum of grad_label rows whose noised label is c, every other row of grad_weight
//                zero.  A workgroup owns a class: it walks noised_labels in chunks of 1024 rows, compacts the chunk's matching
//                rows in ascending order into LDS (a workgroup prefix sum of the per-thread counts), and sums them: the 256
//                threads are `segs` groups of H / 4 (a float4 of columns each), group s taking the s-th contiguous share of the
//                chunk's list, in order; the groups' partial sums are added in group order at the end.  No atomics; the order
//                depends on the labels alone: bitwise reproducible.
#include "msda_attn_tile.h"
#include "msda_common.h"
#include "msda_launch.h"

// The key noise must give the bits of its restatement in separate torch ops: no product may be fused into the sum that follows
// it.  (__fmul_rn / __fadd_rn would not do: the compiler's HIP headers define them as the plain operators, contractable like
// any other, and a first form of this file written with them differed from torch in the last bit.)
#pragma clang fp contract(off)

namespace msda {

namespace {

constexpr int kCdnBlock = 256;
constexpr int kCdnRows = kCdnBlock / kWave;    // forward: a wavefront per output row
constexpr int kCdnChunk = 4 * kCdnBlock;       // backward: rows of noised_labels per compaction

struct CdnFwdArgs {
    const int64_t *labels, *offsets;
    const float *keys, *weight;
    const long long *seed;
    float *out_label, *out_key, *key_debug;
    int32_t *noised;
    long long T, rows_book, rows;              // rows = B * pad
    int W, H, single_pad, pad, num_classes;
    unsigned thr;
    float scale;
};

__global__ __launch_bounds__(kCdnBlock) void cdn_prepare_fwd_kernel(CdnFwdArgs a)
{
    const int lane = threadIdx.x & (kWave - 1);
    const long long row = (long long)blockIdx.x * kCdnRows + (threadIdx.x >> 6);     // wave-uniform
    if (row >= a.rows) return;
    const int b = (int)(row / a.pad), p = (int)(row % a.pad);
    const int r = p / a.single_pad, j = p % a.single_pad;
    const long long o0 = a.offsets[b], o1 = a.offsets[b + 1];
    const long long t = o0 + j;
    bool live = o0 >= 0 && o1 >= o0 && j < o1 - o0 && t < a.T;
    const bool draws = a.thr != 0u || a.scale > 0.f;
    const unsigned base = draws ? at_mix((unsigned long long)a.seed[0], 0u) : 0u;
    const unsigned e = (unsigned)((long long)r * a.T + t);                             // < E < 2^32 (checked by the host)
    long long lab = -1;
    if (live) {
        lab = a.labels[t];
        if (a.thr != 0u && at_hash(base + 2u * e) < a.thr)
            lab = (long long)(((unsigned long long)at_hash(base + 2u * e + 1u) * (unsigned long long)a.num_classes) >> 32);
        live = lab >= 0 && lab < a.rows_book;
        if (!live) lab = -1;
    }
    if (lane == 0) a.noised[row] = (int32_t)lab;

    float4 *dst = reinterpret_cast<float4 *>(a.out_label + row * a.H);
    const float4 *src = reinterpret_cast<const float4 *>(a.weight + (live ? lab : 0) * a.H);
    for (int q = lane; q < a.H / 4; q += kWave) dst[q] = live ? src[q] : make_float4(0.f, 0.f, 0.f, 0.f);

    for (int c = lane; c < a.W; c += kWave) {
        float v = 0.f, noisy = 0.f;
        if (live) {
            float key = a.keys[t * a.W + c];
            if (a.scale > 0.f) {
                const unsigned E = (unsigned)(2 * (a.pad / (2 * a.single_pad)) * a.T);
                const unsigned k = 2u * E + 2u * (e * (unsigned)a.W + (unsigned)c);
                const float sign = (at_hash(base + k) >> 31) ? 1.f : -1.f;
                const float u = (float)(at_hash(base + k + 1u) >> 8) * 5.9604644775390625e-8f;      // exact: 24 bits * 2^-24
                const float part = (u + ((r & 1) ? 1.f : 0.f)) * sign;
                const float step = (part * key) * a.scale;                              // three roundings, as three torch kernels
                key = key + step;                                                       // (contraction is off in this file)
                key = key != key ? key : fminf(fmaxf(key, 0.f), 1.f);                  // torch.clamp: NaN stays
            }
            noisy = key;
            v = inverse_sigmoid_f32(key);
        }
        a.out_key[row * a.W + c] = v;
        if (a.key_debug != nullptr) a.key_debug[row * a.W + c] = noisy;
    }
}

// Inclusive prefix sum of one int per thread over the workgroup (4 wavefronts): shuffles inside a wavefront, the wavefronts'
// totals through LDS.  Returns the thread's inclusive sum; *total = the workgroup's.
__device__ __forceinline__ int cdn_block_scan(int v, int *wave_tot, int *total)
{
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
#pragma unroll
    for (int s = 1; s < kWave; s <<= 1) {
        const int up = __shfl_up(v, s, kWave);
        if (lane >= s) v += up;
    }
    __syncthreads();                                                                    // the previous chunk's readers are done
    if (lane == kWave - 1) wave_tot[wave] = v;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kCdnBlock / kWave; ++w) {
        const int x = wave_tot[w];
        before += w < wave ? x : 0;
        all += x;
    }
    *total = all;
    return v + before;
}

__global__ __launch_bounds__(kCdnBlock) void cdn_prepare_bwd_kernel(const float *__restrict__ grad, const int32_t *__restrict__ noised,
                                                                    long long rows, int H, float *__restrict__ gw)
{
    __shared__ int list[kCdnChunk];
    __shared__ int wave_tot[kCdnBlock / kWave];
    __shared__ __attribute__((aligned(16))) float4 part[kCdnBlock];
    const int tid = threadIdx.x, cls = blockIdx.x;
    const int nvec = H / 4, segs = kCdnBlock / nvec;                                   // H <= 1024: segs >= 1
    const int seg = tid / nvec, col = tid % nvec;
    const bool worker = seg < segs;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (long long c0 = 0; c0 < rows; c0 += kCdnChunk) {
        // the chunk's matching rows in ascending order: thread tid looks at rows c0 + 4 tid .. + 3
        const long long r0 = c0 + 4 * tid;
        int hit[4], n = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            hit[k] = (r0 + k < rows && noised[r0 + k] == cls) ? 1 : 0;
            n += hit[k];
        }
        int count;
        int at = cdn_block_scan(n, wave_tot, &count) - n;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (hit[k]) list[at++] = 4 * tid + k;
        __syncthreads();
        if (worker) {
            const int share = (count + segs - 1) / segs;
            const int i0 = seg * share, i1 = min(count, i0 + share);
            for (int i = i0; i < i1; ++i) {
                const float4 g = reinterpret_cast<const float4 *>(grad + (c0 + list[i]) * H)[col];
                acc.x += g.x; acc.y += g.y; acc.z += g.z; acc.w += g.w;
            }
        }
    }
    part[tid] = acc;
    __syncthreads();
    if (tid < nvec) {
        float4 s = part[tid];
        for (int k = 1; k < segs; ++k) {
            const float4 g = part[k * nvec + tid];
            s.x += g.x; s.y += g.y; s.z += g.z; s.w += g.w;
        }
        reinterpret_cast<float4 *>(gw + (long long)cls * H)[tid] = s;
    }
}

}  // namespace

int launch_cdn_prepare_fwd(const int64_t *labels, const int64_t *offsets, const float *keys, const float *weight, const long long *seed,
                           int B, long long T, int W, int H, long long rows_book, int single_pad, int groups, int num_classes,
                           unsigned thr, float scale, float *out_label, float *out_key, int32_t *noised, float *key_debug,
                           hipStream_t stream)
{
    CdnFwdArgs a;
    a.labels = labels; a.offsets = offsets; a.keys = keys; a.weight = weight; a.seed = seed;
    a.out_label = out_label; a.out_key = out_key; a.key_debug = key_debug; a.noised = noised;
    a.T = T; a.rows_book = rows_book;
    a.W = W; a.H = H; a.single_pad = single_pad; a.pad = 2 * single_pad * groups; a.num_classes = num_classes;
    a.rows = (long long)B * a.pad;
    a.thr = thr; a.scale = scale;
    if (a.rows == 0) return MSDA_OK;
    hipLaunchKernelGGL(cdn_prepare_fwd_kernel, dim3((unsigned)((a.rows + kCdnRows - 1) / kCdnRows)), dim3(kCdnBlock), 0, stream, a);
    return check_launch("cdn_prepare_fwd_kernel");
}

int launch_cdn_prepare_bwd(const float *grad_label, const int32_t *noised, long long rows, int H, long long rows_book, float *grad_weight,
                           hipStream_t stream)
{
    if (rows_book == 0) return MSDA_OK;
    hipLaunchKernelGGL(cdn_prepare_bwd_kernel, dim3((unsigned)rows_book), dim3(kCdnBlock), 0, stream, grad_label, noised, rows, H,
                       grad_weight);
    return check_launch("cdn_prepare_bwd_kernel");
}

}  // namespace msda
