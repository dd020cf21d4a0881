// Two-stage query selection of UVHand's DINO DeformableTransformer (models/dino/deformable_transformer.py:348-387) for any
// number of encoder rows per frame:
//
//   keys      one thread per row: the row's max / argmax over the K class logits (torch.max(-1) / argmax(-1): first maximum,
//             NaN wins), a 64-bit key (~float_order(max) << 32) | row — unique per row, ascending key = descending max, then
//             ascending row — and the row's code byte (2 hand, 1 object, 0 neither) to the workspace, and slot[n, s] = -1.
//   select    one 1024-thread workgroup per frame: a radix select (8-bit digits from the top, LDS histograms, integer LDS
//             atomics) for the Q-th smallest key, the Q keys at or below it compacted into LDS (arrival order — harmless, they
//             are sorted next), a bitonic sort of <= 2048 keys, then topk, slot, code and the gathered rows of `memory`
//             (float4) and `proposals`.  The keys are read from the workspace (N * S * 8 bytes: L2-resident at model sizes).
//   backward  grad_memory[n, s, :] = slot[n, s] >= 0 ? grad_tgt[n, slot[n, s], :] : 0 — every element written, float4 per
//             thread, no memset, no atomics, no scatter.
//
// The rule is msda_two_stage_select_f32's (msda_two_stage.hip), which sorts the whole frame in LDS and stops at 8192 rows.
// Nothing here depends on arrival order: the threshold is a property of the key set, and the order is a sort of unique keys.
#include "msda_common.h"
#include "msda_launch.h"

namespace msda {

constexpr int kDsBlock = 256;                  // keys / backward
constexpr int kDsSelBlock = 1024;              // select: one workgroup per frame

// order-preserving image of a float as an unsigned integer; NaN above +inf, -0 == +0 (as msda_two_stage.hip)
__device__ __forceinline__ uint32_t ds_float_order(float x)
{
    if (x != x) return 0xffffffffu;
    if (x == 0.f) x = 0.f;
    const uint32_t b = __float_as_uint(x);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// grid (ceil(S / 256), N)
__global__ __launch_bounds__(kDsBlock) void dino_select_keys_kernel(
    const float *__restrict__ cls, int S, int K, int hand0, int hand1, unsigned long long *__restrict__ keys,
    uint8_t *__restrict__ row_code, int32_t *__restrict__ slot)
{
    const int s = blockIdx.x * kDsBlock + threadIdx.x;
    if (s >= S) return;
    const long long row = (long long)blockIdx.y * S + s;
    const float *p = cls + row * K;
    float mx = p[0];
    int arg = 0;
    for (int k = 1; k < K; ++k) {
        const float v = p[k];
        if (mx != mx) break;
        if (v != v || v > mx) { mx = v; arg = k; }
    }
    keys[row] = ((unsigned long long)(~ds_float_order(mx)) << 32) | (unsigned)s;
    const bool is_hand = arg == hand0 || arg == hand1;
    row_code[row] = is_hand ? 2 : (arg != 0 ? 1 : 0);
    slot[row] = -1;
}

// grid (N); P = the power of two >= max(Q, 2)
__global__ __launch_bounds__(kDsSelBlock) void dino_select_kernel(
    const unsigned long long *__restrict__ keys, const uint8_t *__restrict__ row_code, const float *__restrict__ memory,
    const float *__restrict__ proposals, int S, int Q, int C, int P, int64_t *__restrict__ topk, int32_t *__restrict__ slot,
    float *__restrict__ tgt, float *__restrict__ prop_sel, uint8_t *__restrict__ code)
{
    __shared__ unsigned long long cand[kDinoSelMaxQueries];
    __shared__ unsigned hist[256];
    __shared__ unsigned wave_total[4];
    __shared__ unsigned long long sh_prefix;
    __shared__ unsigned sh_rank, sh_done, sh_count;
    const int n = blockIdx.x, tid = threadIdx.x;
    const unsigned long long *kf = keys + (long long)n * S;

    // ---- the Q-th smallest key.  Invariant: exactly `rank` of the wanted keys lie among those that match `prefix` on the
    // bits above the current digit; the digits of the row index that no row below S can set are skipped (always 0).
    unsigned long long prefix = 0, thr = ~0ull;
    unsigned rank = (unsigned)Q;
    bool done = false;
    for (int shift = 56; shift >= 0 && !done; shift -= 8) {
        if (shift < 32 && (((unsigned)(S - 1)) >> shift) == 0u && shift > 0) continue;
        const unsigned long long above = shift == 56 ? 0ull : (~0ull << (shift + 8));
        if (tid < 256) hist[tid] = 0u;
        __syncthreads();
        for (int s = tid; s < S; s += kDsSelBlock) {
            const unsigned long long k = kf[s];
            if ((k & above) == prefix) atomicAdd(&hist[(unsigned)(k >> shift) & 255u], 1u);
        }
        __syncthreads();
        // inclusive scan of the 256 counts: a shuffle scan inside each of the first four wavefronts, then their totals
        unsigned own = 0u, cum = 0u;
        if (tid < 256) {
            own = hist[tid];
            cum = own;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned up = __shfl_up(cum, d, 64);
                if ((tid & 63) >= d) cum += up;
            }
            if ((tid & 63) == 63) wave_total[tid >> 6] = cum;
        }
        __syncthreads();
        if (tid < 256) {
            for (int w = 0; w < (tid >> 6); ++w) cum += wave_total[w];
            if (cum >= rank && cum - own < rank) {                   // exactly one bucket holds the rank-th key
                sh_prefix = prefix | ((unsigned long long)tid << shift);
                sh_rank = rank - (cum - own);
                sh_done = cum == rank ? 1u : 0u;                      // every key of this bucket is wanted: no need to go deeper
            }
        }
        __syncthreads();
        prefix = sh_prefix;
        rank = sh_rank;
        if (sh_done || shift == 0) {
            thr = prefix | (shift == 0 ? 0ull : ((1ull << shift) - 1ull));
            done = true;
        }
        __syncthreads();                                             // sh_* are rewritten by the next digit
    }

    // ---- the Q keys at or below the threshold, then padding that sorts last (no real key has an all-ones high word)
    if (tid == 0) sh_count = 0u;
    for (int i = Q + tid; i < P; i += kDsSelBlock) cand[i] = ~0ull;
    __syncthreads();
    for (int s = tid; s < S; s += kDsSelBlock) {
        const unsigned long long k = kf[s];
        if (k <= thr) {
            const unsigned at = atomicAdd(&sh_count, 1u);
            if (at < (unsigned)Q) cand[at] = k;                      // at < Q always (keys are unique); the guard keeps LDS safe
        }
    }
    __syncthreads();
    // bitonic sort, ascending: descending max, then ascending row index
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < P / 2; t += kDsSelBlock) {
                const int i = 2 * t - (t & (j - 1)), ixj = i + j;
                const unsigned long long a = cand[i], b = cand[ixj];
                const bool up = (i & k) == 0;
                if ((a > b) == up) { cand[i] = b; cand[ixj] = a; }
            }
            __syncthreads();
        }
    }

    // ---- outputs
    const long long base = (long long)n * S, qbase = (long long)n * Q;
    for (int q = tid; q < Q; q += kDsSelBlock) {
        const int s = (int)(cand[q] & 0xffffffffu);
        topk[qbase + q] = s;
        slot[base + s] = q;
        code[qbase + q] = row_code[base + s];
    }
    const int per_row = C / 4;
    const float4 *mem4 = reinterpret_cast<const float4 *>(memory);
    float4 *tgt4 = reinterpret_cast<float4 *>(tgt);
    for (int e = tid; e < Q * per_row; e += kDsSelBlock) {
        const int q = e / per_row, c4 = e % per_row;
        const int s = (int)(cand[q] & 0xffffffffu);
        tgt4[(qbase + q) * per_row + c4] = mem4[(base + s) * per_row + c4];
    }
    for (int e = tid; e < Q * 42; e += kDsSelBlock) {
        const int q = e / 42, col = e % 42;
        const int s = (int)(cand[q] & 0xffffffffu);
        prop_sel[(qbase + q) * 42 + col] = proposals[(base + s) * 42 + col];
    }
}

// one thread per float4 of grad_memory
__global__ __launch_bounds__(kDsBlock) void dino_select_bwd_kernel(
    const int32_t *__restrict__ slot, const float *__restrict__ grad_tgt, int S, int Q, int per_row, long long total,
    float *__restrict__ grad_memory)
{
    const long long e = (long long)blockIdx.x * kDsBlock + threadIdx.x;
    if (e >= total) return;
    const long long row = e / per_row;
    const int c4 = (int)(e % per_row);
    const int q = slot[row];
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (q >= 0) v = reinterpret_cast<const float4 *>(grad_tgt)[((row / S) * Q + q) * per_row + c4];
    reinterpret_cast<float4 *>(grad_memory)[e] = v;
}

size_t dino_select_workspace_bytes(int N, int S)
{
    const size_t rows = (size_t)N * (size_t)S;
    return rows * 8 + ((rows + 15) & ~(size_t)15);                  // the keys, then the code bytes
}

int launch_dino_select_fwd(const float *cls, const float *memory, const float *proposals, int N, int S, int K, int Q, int C,
                           int hand0, int hand1, int64_t *topk, int32_t *slot, float *tgt, float *prop_sel, uint8_t *code,
                           void *workspace, hipStream_t stream)
{
    if (N == 0) return MSDA_OK;
    unsigned long long *keys = static_cast<unsigned long long *>(workspace);
    uint8_t *row_code = static_cast<uint8_t *>(workspace) + (size_t)N * S * 8;
    hipLaunchKernelGGL(dino_select_keys_kernel, dim3((unsigned)((S + kDsBlock - 1) / kDsBlock), (unsigned)N), dim3(kDsBlock), 0, stream,
                       cls, S, K, hand0, hand1, keys, row_code, slot);
    int P = 2;
    while (P < Q) P <<= 1;
    hipLaunchKernelGGL(dino_select_kernel, dim3((unsigned)N), dim3(kDsSelBlock), 0, stream, keys, row_code, memory, proposals, S, Q, C,
                       P, topk, slot, tgt, prop_sel, code);
    return check_launch("dino_select_kernel");
}

int launch_dino_select_bwd(const int32_t *slot, const float *grad_tgt, int N, int S, int Q, int C, float *grad_memory,
                           hipStream_t stream)
{
    if (N == 0) return MSDA_OK;
    const int per_row = C / 4;
    const long long total = (long long)N * S * per_row;
    hipLaunchKernelGGL(dino_select_bwd_kernel, dim3((unsigned)((total + kDsBlock - 1) / kDsBlock)), dim3(kDsBlock), 0, stream, slot,
                       grad_tgt, S, Q, per_row, total, grad_memory);
    return check_launch("dino_select_bwd_kernel");
}

}  // namespace msda
