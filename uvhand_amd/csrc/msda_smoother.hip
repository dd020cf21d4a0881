// SmoothNet's MotionSmoother (UVHand models/smoothnet.py:7-125) as grouped fp32 GEMMs: every Smoother of every module that a
// set of calls uses, in one launch per MLP depth forward, and in at most 11 launches backward.
//
// A module is one MotionSmoother: three Smoothers (pos / vel / acc, window T, T - 1, T - 2) and the fusion Linear(3 O, O).
// Its rows are the (b, c) rows of every call that uses it, concatenated in call order: call i (input x [B_i * T, C_i], i.e.
// x.view(B, T, C).permute(0, 2, 1)) owns module rows [row0_i, row0_i + B_i * C_i), row = row0_i + b * C_i + c.  A problem
// is one Smoother of one module (its layers, in order: l = 0 encoder Linear(T', H) + LeakyReLU(0.1); l = 2j - 1 and 2j the
// two Linears of residual block j = 1..nb, each with the epilogue dropout -> LeakyReLU(0.2), the second adding the block's
// input; l = 2 nb + 1 the decoder Linear(H, O)), or the fusion Linear of one module (s = 3).
//
//   forward   depth l of every Smoother problem, then the fusion: 2 nb + 3 launches.  The encoder stages its A operand straight
//             from the call's input ([B * T, C], permuted and differenced on the fly: vel = x[t + 1] - x[t], acc = vel[t + 1] -
//             vel[t] of the ROUNDED vel values, as the reference computes them); the decoders write the module's [rows, 3 O]
//             concatenation (cat order pos, vel, acc), the fusion's K loop runs over it and its epilogue writes the call's
//             [B * O, C] output.  Saved for the backward: every layer's output after its epilogue (and, per block, the
//             pre-residual value), [rows, .] per problem.
//   dgrad     input gradients depth by depth from the fusion down to the encoder (whose launch is skipped when no call's
//             input wants a gradient): dx = (dy o mode) . W, mode = LeakyReLU' from the saved output and the regenerated
//             dropout mask; the first Linear of a block adds the residual's gradient in its epilogue.
//   wgrad     one launch: dW = (dy o mode)^T . x for every layer of every problem over all of its rows (the rows of calls
//             that share a module reduce together), the bias sums beside it; written straight into the flat gradient
//             buffer (parameters in the module's parameters() order).
//   fold      (only with input gradients) one launch: the encoders' pos / vel / acc adjoints back onto one [B * T, C]
//             gradient per call.
//
// Dropout (training): keep iff the top 32 bits of a 64-bit hash of (64-bit seed, problem, layer, row, column) are >= p * 2^32;
// kept values are scaled by 1 / (1 - p).  The seed is read from device memory (drawn by the caller from torch's generator);
// the backward regenerates the mask.  The stream is not nn.Dropout's.
// Kernels: the grouped 64 x 64 fp32-MFMA tile of msda_tile.h.  Fixed summation order everywhere, no atomics: bitwise
// reproducible.
#include <cstdio>
#include <cstring>

#include "msda_common.h"
#include "msda_launch.h"

namespace msda {

namespace {

#include "msda_tile.h"

constexpr int kSmMaxMods = 6, kSmMaxCalls = 12, kSmMaxCallsPerMod = 4, kSmMaxBlocks = 4, kSmMaxJobs = 192;

struct SmCall {                 // one call: input x [B * T, C], output out [B * O, C], their gradients (backward)
    const float *x;
    float *out;
    const float *gout;
    float *gx;
    int B, C, mod, row0;
};
struct SmMod {                  // one module: its rows, its calls (row0 ascending), its offsets in the three buffers
    int rows, ncalls, calls[kSmMaxCallsPerMod];
    long long act, dws, gp;
};
struct SmGeo {
    SmCall c[kSmMaxCalls];
    SmMod m[kSmMaxMods];
    float *act, *ws, *gp;                       // saved activations, backward workspace, flat parameter gradients
    const unsigned long long *seed;             // device; read only when train
    int T, O, H, R, nb, nmod, ncalls, train;
    unsigned thresh;                            // keep iff hash >= thresh (p * 2^32)
    float scale;                                // 1 / (1 - p)
};

struct SmFwdProb {
    const float *w, *b;
    int tile0, m, s;
};
struct SmFwdArgs {
    SmGeo G;
    SmFwdProb p[3 * kSmMaxMods];
    int nprob, l;
};
struct SmDgradProb {
    const float *w;
    int tile0, m, s;
};
struct SmDgradArgs {
    SmGeo G;
    SmDgradProb p[3 * kSmMaxMods];
    int nprob, l;
};
struct SmJob {
    int tile0;
    int msl;                                    // (module * 4 + s) << 8 | layer; s = 3: the fusion
};
struct SmWgradArgs {
    SmGeo G;
    SmJob j[kSmMaxJobs];
    int njobs;
};
struct SmFoldArgs {
    SmGeo G;
    int blk0[kSmMaxCalls + 1];
};
static_assert(sizeof(SmFwdArgs) <= 4000 && sizeof(SmDgradArgs) <= 4000 && sizeof(SmWgradArgs) <= 4000
              && sizeof(SmFoldArgs) <= 4000, "kernel argument tables");

// ---- dropout hash ----------------------------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ unsigned long long sm_fmix64(unsigned long long k)
{
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdULL;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ULL;
    k ^= k >> 33;
    return k;
}

// all 64 seed bits and the coordinates (problem < 2^10, layer < 2^6, row < 2^24, column < 2^24) through the 64-bit finaliser
__device__ __forceinline__ bool sm_keep(unsigned long long seed, int prob, int layer, int row, int col, unsigned thresh)
{
    const unsigned long long coord = ((unsigned long long)(prob * 64 + layer) << 48) ^ ((unsigned long long)row << 24)
                                     ^ (unsigned long long)col;
    const unsigned long long h = sm_fmix64(sm_fmix64(seed ^ 0x9E3779B97F4A7C15ULL) + sm_fmix64(coord ^ 0xD1B54A32D192ED03ULL));
    return (unsigned)(h >> 32) >= thresh;
}

// ---- geometry ------------------------------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ int sm_fusion_layer(int nb) { return 2 * nb + 2; }
__host__ __device__ __forceinline__ int sm_layer_k(int T, int O, int H, int R, int nb, int s, int l)
{
    if (s == 3) return 3 * O;
    if (l == 0) return T - s;
    if (l == 2 * nb + 1) return H;
    return (l & 1) ? H : R;
}
__host__ __device__ __forceinline__ int sm_layer_n(int T, int O, int H, int R, int nb, int s, int l)
{
    if (s == 3 || l == 2 * nb + 1) return O;
    if (l == 0) return H;
    return (l & 1) ? R : H;
}
// floats of one Smoother's parameters, and the offset of layer l's weight (its bias follows it) in the module's flat layout
__host__ __device__ __forceinline__ long long sm_smoother_params(int T, int O, int H, int R, int nb, int s)
{
    return (long long)H * (T - s) + H + (long long)nb * (2LL * R * H + R + H) + (long long)O * H + O;
}
__host__ __device__ __forceinline__ long long sm_param_off(int T, int O, int H, int R, int nb, int s, int l)
{
    long long off = 0;
    for (int t = 0; t < (s < 3 ? s : 3); ++t) off += sm_smoother_params(T, O, H, R, nb, t);
    if (s == 3 || l == 0) return off;
    off += (long long)H * (T - s) + H;
    if (l == 2 * nb + 1) return off + (long long)nb * (2LL * R * H + R + H);
    const int j = (l + 1) / 2;
    off += (long long)(j - 1) * (2LL * R * H + R + H);
    return (l & 1) ? off : off + (long long)R * H + R;
}
__host__ __device__ __forceinline__ long long sm_module_params(int T, int O, int H, int R, int nb)
{
    return sm_param_off(T, O, H, R, nb, 3, 0) + 3LL * O * O + O;
}
// per-row floats: activations of one Smoother, backward workspace of one Smoother
__host__ __device__ __forceinline__ long long sm_act_stride(int H, int R, int nb) { return H + (long long)nb * (R + 2 * H); }
__host__ __device__ __forceinline__ long long sm_ws_stride(int H, int R, int nb) { return (long long)(nb + 1) * H + (long long)nb * R; }
__host__ __device__ __forceinline__ long long sm_act_floats(int T, int O, int H, int R, int nb, long long rows)
{
    return rows * (3 * sm_act_stride(H, R, nb) + 3LL * O);
}
__host__ __device__ __forceinline__ long long sm_ws_floats(int T, int O, int H, int R, int nb, long long rows)
{
    return rows * (3 * sm_ws_stride(H, R, nb) + 3LL * O + 3LL * T);
}

// activations of module m (rows Rm): h(s, j) [Rm, H] (j = 0: the encoder's output), u(s, j) [Rm, R], g(s, j) [Rm, H] (block j's
// value before the residual), D [Rm, 3 O]
struct SmAct {
    float *base;
    long long rows, S;
    int H, R;
    __device__ float *h(int s, int j) const
    {
        return base + rows * (s * S + (j == 0 ? 0 : H + (long long)(j - 1) * (R + 2 * H) + R + H));
    }
    __device__ float *u(int s, int j) const { return base + rows * (s * S + H + (long long)(j - 1) * (R + 2 * H)); }
    __device__ float *g(int s, int j) const { return u(s, j) + rows * R; }
    __device__ float *D() const { return base + rows * 3 * S; }
};
__device__ __forceinline__ SmAct sm_act(const SmGeo &G, int m)
{
    return SmAct{G.act + G.m[m].act, G.m[m].rows, sm_act_stride(G.H, G.R, G.nb), G.H, G.R};
}
// backward workspace of module m: dH(s, j) [Rm, H], dU(s, j) [Rm, R], dD [Rm, 3 O], dX(s) [Rm, T - s]
struct SmWs {
    float *base;
    long long rows, S;
    int H, R, nb, O, T;
    __device__ float *dH(int s, int j) const { return base + rows * (s * S + (long long)j * H); }
    __device__ float *dU(int s, int j) const { return base + rows * (s * S + (long long)(nb + 1) * H + (long long)(j - 1) * R); }
    __device__ float *dD() const { return base + rows * 3 * S; }
    __device__ float *dX(int s) const { return base + rows * (3 * S + 3LL * O + (long long)T * s); }
};
__device__ __forceinline__ SmWs sm_ws(const SmGeo &G, int m)
{
    return SmWs{G.ws + G.m[m].dws, G.m[m].rows, sm_ws_stride(G.H, G.R, G.nb), G.H, G.R, G.nb, G.O, G.T};
}

// the call that owns module row r, and (b, c) within it
__device__ __forceinline__ const SmCall &sm_row_call(const SmGeo &G, int m, int r, int &b, int &c)
{
    int k = 0;                                  // a module's calls lie in call order, row0 ascending: the last one that starts <= r
    for (int i = 0; i < G.ncalls; ++i)
        if (G.c[i].mod == m && r >= G.c[i].row0) k = i;
    const SmCall &C = G.c[k];
    const int rr = r - C.row0;
    b = rr / C.C;
    c = rr - b * C.C;
    return C;
}

// the call operands of module row r: its input column x[b, :, c] and output-gradient column gout[b, :, c] (stride C)
struct SmRowRef {
    const float *x, *g;
    long long st;
};
__device__ __forceinline__ SmRowRef sm_row_ref(const SmGeo &G, int m, int r)
{
    int b, c;
    const SmCall &C = sm_row_call(G, m, r, b, c);
    SmRowRef R;
    R.x = C.x ? C.x + (long long)b * G.T * C.C + c : nullptr;
    R.g = C.gout ? C.gout + (long long)b * G.O * C.C + c : nullptr;
    R.st = C.C;
    return R;
}

// layer l's input at (row r, column k) of problem (m, s): the permuted / differenced call input for the encoder (from `rr`,
// row r's SmRowRef)
__device__ __forceinline__ float sm_x_at(const SmGeo &G, int m, int s, int l, int r, int k, const SmRowRef &rr)
{
    if (s == 3) return sm_act(G, m).D()[(long long)r * 3 * G.O + k];
    if (l == 0) {
        const float *x = rr.x;
        const long long st = rr.st;
        if (s == 0) return x[k * st];
        const float x0 = x[k * st], x1 = x[(k + 1) * st];
        const float v0 = x1 - x0;
        if (s == 1) return v0;
        const float v1 = x[(k + 2) * st] - x1;
        return v1 - v0;
    }
    const SmAct A = sm_act(G, m);
    if (l == 2 * G.nb + 1) return A.h(s, G.nb)[(long long)r * G.H + k];
    if (l & 1) return A.h(s, (l - 1) / 2)[(long long)r * G.H + k];
    return A.u(s, l / 2)[(long long)r * G.R + k];
}

// the gradient at layer l's OUTPUT, through its epilogue (LeakyReLU' from the saved output, the dropout mask): (row r, col i)
__device__ __forceinline__ float sm_dy_at(const SmGeo &G, int m, int s, int l, int r, int i, const SmRowRef &rr)
{
    if (s == 3) return rr.g[i * rr.st];
    const SmWs W = sm_ws(G, m);
    if (l == 2 * G.nb + 1) return W.dD()[(long long)r * 3 * G.O + s * G.O + i];
    const SmAct A = sm_act(G, m);
    if (l == 0) {
        const long long e = (long long)r * G.H + i;
        const float g = W.dH(s, 0)[e];
        return A.h(s, 0)[e] > 0.f ? g : g * 0.1f;
    }
    const int j = (l + 1) / 2;
    const bool first = (l & 1) != 0;
    const long long e = (long long)r * (first ? G.R : G.H) + i;
    const float g = first ? W.dU(s, j)[e] : W.dH(s, j)[e];
    const float y = first ? A.u(s, j)[e] : A.g(s, j)[e];
    float v = y > 0.f ? g : g * 0.2f;
    if (G.train) v = sm_keep(G.seed[0], m * 3 + s, l, r, i, G.thresh) ? v * G.scale : 0.f;
    return v;
}

// ---- forward: one depth of every problem ----------------------------------------------------------------------------------
template <bool MID>
__global__ __launch_bounds__(kHBlock) void sm_fwd_kernel(SmFwdArgs P)
{
    __shared__ __attribute__((aligned(16))) float As[2][kLds];
    __shared__ __attribute__((aligned(16))) float Bs[2][kLds];
    int pi = 0;
    while (pi + 1 < P.nprob && (int)blockIdx.x >= P.p[pi + 1].tile0) ++pi;
    const SmFwdProb &p = P.p[pi];
    const SmGeo &G = P.G;
    const int m = p.m, s = p.s, l = P.l, rows = G.m[m].rows, tid = threadIdx.x;
    const int K = sm_layer_k(G.T, G.O, G.H, G.R, G.nb, s, l), n = sm_layer_n(G.T, G.O, G.H, G.R, G.nb, s, l);
    const int tiles_n = (n + kHT - 1) / kHT;
    const int local = (int)blockIdx.x - p.tile0;
    if (local >= ((rows + kHT - 1) / kHT) * tiles_n) return;
    const int m0 = (local / tiles_n) * kHT, n0 = (local % tiles_n) * kHT;
    const SmAct A = sm_act(G, m);
    const float *X = nullptr;
    if (MID) X = l == 2 * G.nb + 1 ? A.h(s, G.nb) : (l & 1) ? A.h(s, (l - 1) / 2) : A.u(s, l / 2);

    auto load = [&](int st, float (&ra)[8], float (&rb)[8]) {
        if (MID) {                                                  // K % 4 == 0: 16-byte K-major
            const int k = st * kHS + (tid % 8) * 4;
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int r = m0 + tid / 8 + 32 * u, j = n0 + tid / 8 + 32 * u;
                float4 va = make_float4(0.f, 0.f, 0.f, 0.f), vb = va;
                if (r < rows && k < K) va = *reinterpret_cast<const float4 *>(X + (long long)r * K + k);
                if (j < n && k < K) vb = *reinterpret_cast<const float4 *>(p.w + (long long)j * K + k);
                ra[4 * u] = va.x; ra[4 * u + 1] = va.y; ra[4 * u + 2] = va.z; ra[4 * u + 3] = va.w;
                rb[4 * u] = vb.x; rb[4 * u + 1] = vb.y; rb[4 * u + 2] = vb.z; rb[4 * u + 3] = vb.w;
            }
        } else {                                                    // encoder (T', virtual input) / fusion (3 O): 4-byte
            const int k = st * kHS + tid % 32;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int r = m0 + tid / 32 + 8 * u, j = n0 + tid / 32 + 8 * u;
                SmRowRef rr{nullptr, nullptr, 1};
            if (l == 0 && s < 3 && r < rows) rr = sm_row_ref(G, m, r);
                ra[u] = (r < rows && k < K) ? sm_x_at(G, m, s, l, r, k, rr) : 0.f;
                rb[u] = (j < n && k < K) ? p.w[(long long)j * K + k] : 0.f;
            }
        }
    };
    const f32x16 acc = tile_loop<true, MID, true, MID>(As, Bs, (K + kHS - 1) / kHS, load, NoStage());

    const int wave = tid >> 6, lane = tid & 63;
    const int i0 = (wave >> 1) * 32, g = lane >> 5, j = n0 + (wave & 1) * 32 + (lane & 31);
    if (j >= n) return;
    const float bj = p.b[j];
    const bool fus = s == 3, dec = !fus && l == 2 * G.nb + 1, enc = !fus && l == 0;
    const int jb = (l + 1) / 2;
    const unsigned long long seed = (!fus && !dec && !enc && G.train) ? G.seed[0] : 0ull;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = m0 + i0 + acc_row(r, g);
        if (row >= rows) continue;
        float v = acc[r] + bj;
        if (fus) {
            int b, c;
            const SmCall &C = sm_row_call(G, m, row, b, c);
            C.out[((long long)b * G.O + j) * C.C + c] = v;
        } else if (dec) {
            A.D()[(long long)row * 3 * G.O + s * G.O + j] = v;
        } else if (enc) {
            A.h(s, 0)[(long long)row * G.H + j] = v > 0.f ? v : v * 0.1f;
        } else {
            if (G.train) v = sm_keep(seed, m * 3 + s, l, row, j, G.thresh) ? v * G.scale : 0.f;
            v = v > 0.f ? v : v * 0.2f;
            if (l & 1) {
                A.u(s, jb)[(long long)row * G.R + j] = v;
            } else {
                const long long e = (long long)row * G.H + j;
                A.g(s, jb)[e] = v;
                A.h(s, jb)[e] = v + A.h(s, jb - 1)[e];
            }
        }
    }
}

// ---- input gradients of one depth: dx [rows, K] = (dy o mode) [rows, n] . W [n, K] -------------------------------------------
template <bool MID>
__global__ __launch_bounds__(kHBlock) void sm_dgrad_kernel(SmDgradArgs P)
{
    __shared__ __attribute__((aligned(16))) float As[2][kLds];
    __shared__ __attribute__((aligned(16))) float Bs[2][kLds];
    int pi = 0;
    while (pi + 1 < P.nprob && (int)blockIdx.x >= P.p[pi + 1].tile0) ++pi;
    const SmDgradProb &p = P.p[pi];
    const SmGeo &G = P.G;
    const int m = p.m, s = p.s, l = P.l, rows = G.m[m].rows, tid = threadIdx.x;
    const int K = sm_layer_k(G.T, G.O, G.H, G.R, G.nb, s, l), n = sm_layer_n(G.T, G.O, G.H, G.R, G.nb, s, l);
    const int tiles_n = (K + kHT - 1) / kHT;
    const int local = (int)blockIdx.x - p.tile0;
    if (local >= ((rows + kHT - 1) / kHT) * tiles_n) return;
    const int m0 = (local / tiles_n) * kHT, n0 = (local % tiles_n) * kHT;

    auto load = [&](int st, float (&ra)[8], float (&rb)[8]) {
        // A = dy o mode [row, k]: 4-byte K-major
        const int k = st * kHS + tid % 32;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int r = m0 + tid / 32 + 8 * u;
            SmRowRef rr{nullptr, nullptr, 1};
            if (s == 3 && r < rows) rr = sm_row_ref(G, m, r);
            ra[u] = (r < rows && k < n) ? sm_dy_at(G, m, s, l, r, k, rr) : 0.f;
        }
        // B = W [k, j]: MN-major
        if (MID) {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int kk = st * kHS + tid / 16 + 16 * u, jn = n0 + (tid % 16) * 4;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (kk < n && jn < K) v = *reinterpret_cast<const float4 *>(p.w + (long long)kk * K + jn);
                rb[4 * u] = v.x; rb[4 * u + 1] = v.y; rb[4 * u + 2] = v.z; rb[4 * u + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int kk = st * kHS + tid / 64 + 4 * u, jn = n0 + tid % 64;
                rb[u] = (kk < n && jn < K) ? p.w[(long long)kk * K + jn] : 0.f;
            }
        }
    };
    const f32x16 acc = tile_loop<true, false, false, MID>(As, Bs, (n + kHS - 1) / kHS, load, NoStage());

    const int wave = tid >> 6, lane = tid & 63;
    const int i0 = (wave >> 1) * 32, g = lane >> 5, j = n0 + (wave & 1) * 32 + (lane & 31);
    if (j >= K) return;
    const SmWs W = sm_ws(G, m);
    const bool fus = s == 3, dec = !fus && l == 2 * G.nb + 1, enc = !fus && l == 0;
    const int jb = (l + 1) / 2;
    float *out = fus ? W.dD() : dec ? W.dH(s, G.nb) : enc ? W.dX(s) : (l & 1) ? W.dH(s, jb - 1) : W.dU(s, jb);
    const float *res = (!fus && !dec && !enc && (l & 1)) ? W.dH(s, jb) : nullptr;   // the block input's identity path
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = m0 + i0 + acc_row(r, g);
        if (row >= rows) continue;
        const long long e = (long long)row * K + j;
        out[e] = res ? acc[r] + res[e] : acc[r];
    }
}

// ---- weight gradients of every layer of every problem: dW [n, K] = (dy o mode)^T . x, db [n] = column sums of dy o mode -------
__global__ __launch_bounds__(kHBlock) void sm_wgrad_kernel(SmWgradArgs P)
{
    __shared__ __attribute__((aligned(16))) float As[2][kLds];
    __shared__ __attribute__((aligned(16))) float Bs[2][kLds];
    __shared__ float bred[4][kHT];
    int ji = 0;
    while (ji + 1 < P.njobs && (int)blockIdx.x >= P.j[ji + 1].tile0) ++ji;
    const int msl = P.j[ji].msl, tile0 = P.j[ji].tile0;
    const SmGeo &G = P.G;
    const int m = msl >> 10, s = (msl >> 8) & 3, l = msl & 255, rows = G.m[m].rows, tid = threadIdx.x;
    const int K = sm_layer_k(G.T, G.O, G.H, G.R, G.nb, s, l), n = sm_layer_n(G.T, G.O, G.H, G.R, G.nb, s, l);
    const int tiles_j = (K + kHT - 1) / kHT, tiles_i = (n + kHT - 1) / kHT;
    const int local = (int)blockIdx.x - tile0;
    if (local >= tiles_i * tiles_j) return;
    const int i0t = (local / tiles_j) * kHT, j0t = (local % tiles_j) * kHT;
    auto load = [&](int st, float (&ra)[8], float (&rb)[8]) {
        // A(i, r) = (dy o mode)[r, i], B(r, k) = x[r, k]: 4-byte MN-major
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int r = st * kHS + tid / 64 + 4 * u, i = i0t + tid % 64, k = j0t + tid % 64;
            SmRowRef rr{nullptr, nullptr, 1};
            if ((l == 0 || s == 3) && r < rows) rr = sm_row_ref(G, m, r);
            ra[u] = (r < rows && i < n) ? sm_dy_at(G, m, s, l, r, i, rr) : 0.f;
            rb[u] = (r < rows && k < K) ? sm_x_at(G, m, s, l, r, k, rr) : 0.f;
        }
    };
    float bsum = 0.f;
    const bool with_bias = j0t == 0;
    auto per_stage = [&](const float *S) {
        if (with_bias) {
            const int i = tid & 63, q = tid >> 6;
#pragma unroll
            for (int u = 0; u < 8; ++u) bsum += S[(8 * q + u) * kRowN + i];
        }
    };
    const f32x16 acc = tile_loop<false, false, false, false>(As, Bs, (rows + kHS - 1) / kHS, load, per_stage);
    float *dw = G.gp + G.m[m].gp + sm_param_off(G.T, G.O, G.H, G.R, G.nb, s, l);
    if (with_bias) {                                                            // uniform per workgroup
        bred[tid >> 6][tid & 63] = bsum;
        __syncthreads();
        if (tid < kHT && i0t + tid < n)
            dw[(long long)n * K + i0t + tid] = ((bred[0][tid] + bred[1][tid]) + bred[2][tid]) + bred[3][tid];
    }
    const int wave = tid >> 6, lane = tid & 63;
    const int i0 = (wave >> 1) * 32, g = lane >> 5, j = j0t + (wave & 1) * 32 + (lane & 31);
    if (j >= K) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int i = i0t + i0 + acc_row(r, g);
        if (i < n) dw[(long long)i * K + j] = acc[r];
    }
}

// ---- the encoders' adjoints back onto each call's input: x -> (pos, vel, acc) transposed ------------------------------------
__global__ __launch_bounds__(kHBlock) void sm_fold_kernel(SmFoldArgs P)
{
    const SmGeo &G = P.G;
    int ci = 0;
    while (ci + 1 < G.ncalls && (int)blockIdx.x >= P.blk0[ci + 1]) ++ci;
    const SmCall &C = G.c[ci];
    if (C.gx == nullptr) return;
    const long long e = (long long)((int)blockIdx.x - P.blk0[ci]) * kHBlock + threadIdx.x;
    const int T = G.T;
    if (e >= (long long)C.B * T * C.C) return;
    const int c = (int)(e % C.C), t = (int)((e / C.C) % T), b = (int)(e / ((long long)C.C * T));
    const SmWs W = sm_ws(G, C.mod);
    const long long r = C.row0 + (long long)b * C.C + c;
    const float *dp = W.dX(0) + r * T, *dv = W.dX(1) + r * (T - 1), *da = W.dX(2) + r * (T - 2);
    // vel's gradient: its own Smoother's, plus acc = vel[1:] - vel[:-1] transposed
    auto dvel = [&](int k) {
        float v = dv[k];
        if (k >= 1) v += da[k - 1];
        if (k <= T - 3) v -= da[k];
        return v;
    };
    float v = dp[t];
    if (t >= 1) v += dvel(t - 1);
    if (t <= T - 2) v -= dvel(t);
    C.gx[e] = v;
}

__global__ __launch_bounds__(kHBlock) void sm_mask_kernel(const unsigned long long *seed, int prob, int layer, int rows, int cols,
                                                          unsigned thresh, float *mask)
{
    const long long e = (long long)blockIdx.x * kHBlock + threadIdx.x;
    if (e >= (long long)rows * cols) return;
    mask[e] = sm_keep(seed[0], prob, layer, (int)(e / cols), (int)(e % cols), thresh) ? 1.f : 0.f;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
// start of an entry that enqueues work: forget this thread's previous message and any sticky error of an unrelated HIP call
void begin_entry()
{
    set_error(MSDA_OK, "");
    (void)hipGetLastError();
}

int serr(const char *msg) { return set_error(MSDA_ERR_ARGUMENT, msg); }

bool sm_dims_ok(int T, int O, int H, int R, int nb)
{
    return T >= 3 && T <= 4096 && O >= 1 && O <= 4096 && H >= 4 && H <= 4096 && H % 4 == 0 && R >= 4 && R <= 4096
           && R % 4 == 0 && nb >= 0 && nb <= kSmMaxBlocks;
}

unsigned sm_thresh(float p) { return p > 0.f ? (unsigned)fmin(4294967295.0, (double)p * 4294967296.0) : 0u; }

// geometry, calls and module offsets; `need_act` / `need_ws`: the buffer sizes (bytes) this call needs
int sm_geometry(SmGeo &G, int T, int O, int H, int R, int nb, int nmod, int ncalls, const int *call_mod, const int *call_B,
                const int *call_C, unsigned long long &need_act, unsigned long long &need_ws)
{
    if (!sm_dims_ok(T, O, H, R, nb))
        return serr("msda_smoother: need 3 <= T <= 4096, 1 <= O <= 4096, hidden sizes H, R in [4, 4096] with H % 4 == R % 4 == 0, "
                    "0 <= num_blocks <= 4");
    if (nmod < 1 || nmod > kSmMaxMods || ncalls < 1 || ncalls > kSmMaxCalls)
        return serr("msda_smoother: need 1 <= modules <= 6 and 1 <= calls <= 12");
    if (call_mod == nullptr || call_B == nullptr || call_C == nullptr) return serr("msda_smoother: null pointer");
    std::memset(&G, 0, sizeof(G));
    G.T = T; G.O = O; G.H = H; G.R = R; G.nb = nb; G.nmod = nmod; G.ncalls = ncalls;
    long long rows[kSmMaxMods] = {};
    for (int i = 0; i < ncalls; ++i) {
        const int m = call_mod[i];
        if (m < 0 || m >= nmod || call_B[i] < 1 || call_C[i] < 1) return serr("msda_smoother: call module out of range or B, C < 1");
        SmMod &M = G.m[m];
        if (M.ncalls == kSmMaxCallsPerMod) return serr("msda_smoother: at most 4 calls per module");
        const long long r = (long long)call_B[i] * call_C[i];
        if ((long long)call_B[i] * T * call_C[i] >= (1LL << 31) || (long long)call_B[i] * O * call_C[i] >= (1LL << 31))
            return serr("msda_smoother: tensors beyond 2^31 elements");
        G.c[i].B = call_B[i]; G.c[i].C = call_C[i]; G.c[i].mod = m; G.c[i].row0 = (int)rows[m];
        M.calls[M.ncalls++] = i;
        rows[m] += r;
        if (rows[m] >= (1LL << 24)) return serr("msda_smoother: more than 2^24 rows in a module");
    }
    const int widest = 3 * (O > H ? (O > R ? O : R) : (H > R ? H : R));
    long long act = 0, ws = 0, gp = 0;
    for (int m = 0; m < nmod; ++m) {
        if (rows[m] * (widest > T ? widest : T) >= (1LL << 31)) return serr("msda_smoother: tensors beyond 2^31 elements");
        G.m[m].rows = (int)rows[m];
        G.m[m].act = act; G.m[m].dws = ws; G.m[m].gp = gp;
        act += sm_act_floats(T, O, H, R, nb, rows[m]);
        ws += sm_ws_floats(T, O, H, R, nb, rows[m]);
        gp += sm_module_params(T, O, H, R, nb);
    }
    need_act = (unsigned long long)act * sizeof(float);
    need_ws = (unsigned long long)ws * sizeof(float);
    return MSDA_OK;
}

int sm_dropout(SmGeo &G, int training, float p, const unsigned long long *seed)
{
    if (!(p >= 0.f && p < 1.f)) return serr("msda_smoother: need 0 <= p < 1");
    G.train = training && p > 0.f;
    if (G.train && seed == nullptr) return serr("msda_smoother: null seed in training mode");
    G.seed = seed;
    G.thresh = sm_thresh(p);
    G.scale = (float)(1.0 / (1.0 - (double)p));
    return MSDA_OK;
}

int params_per_module(int nb) { return 3 * (4 + 4 * nb) + 2; }

// the weight / bias pointer of layer l of smoother s (s = 3: the fusion) of a module's parameter list
const float *sm_param(const float *const *mp, int nb, int s, int l, int bias)
{
    const int per = 4 + 4 * nb;
    return mp[s == 3 ? 3 * per + bias : s * per + 2 * l + bias];
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

int sm_check_params(const SmGeo &G, const float *const *params)
{
    if (params == nullptr) return serr("msda_smoother: null pointer");
    const int per = params_per_module(G.nb);
    for (int i = 0; i < G.nmod * per; ++i)
        if (params[i] == nullptr) return serr("msda_smoother: null pointer");
    for (int m = 0; m < G.nmod; ++m)
        for (int s = 0; s < 3; ++s)
            for (int l = 1; l <= 2 * G.nb + 1; ++l)
                if (!aligned16(sm_param(params + m * per, G.nb, s, l, 0)))
                    return serr("msda_smoother: hidden-layer weights must be 16-byte aligned");
    return MSDA_OK;
}

int sm_tiles(long long rows, int n) { return (int)(((rows + kHT - 1) / kHT) * ((n + kHT - 1) / kHT)); }

}  // namespace

}  // namespace msda

using namespace msda;

extern "C" {

int msda_smoother_supported(int T, int O, int H, int R, int num_blocks) { return sm_dims_ok(T, O, H, R, num_blocks) ? 1 : 0; }

unsigned long long msda_smoother_workspace_bytes(int T, int O, int H, int R, int num_blocks, int n_mod, int n_calls,
                                                 const int *call_mod, const int *call_B, const int *call_C, int which)
{
    static thread_local SmGeo G;
    unsigned long long act = 0, ws = 0;
    if (sm_geometry(G, T, O, H, R, num_blocks, n_mod, n_calls, call_mod, call_B, call_C, act, ws) != MSDA_OK) return 0;
    return which == 0 ? act : which == 1 ? ws : 0;
}

int msda_smoother_forward_f32(int T, int O, int H, int R, int num_blocks, int n_mod, int n_calls, const int *call_mod,
                              const int *call_B, const int *call_C, const float *const *x, const float *const *params,
                              float *const *out, float *act, unsigned long long act_bytes, int training, float p,
                              const unsigned long long *seed, msda_stream_t stream)
{
    static thread_local SmFwdArgs a;
    unsigned long long need_act = 0, need_ws = 0;
    int rc = sm_geometry(a.G, T, O, H, R, num_blocks, n_mod, n_calls, call_mod, call_B, call_C, need_act, need_ws);
    if (rc == MSDA_OK) rc = sm_dropout(a.G, training, p, seed);
    if (rc == MSDA_OK) rc = sm_check_params(a.G, params);
    if (rc != MSDA_OK) return rc;
    if (x == nullptr || out == nullptr || act == nullptr) return serr("msda_smoother: null pointer");
    for (int i = 0; i < n_calls; ++i)
        if (x[i] == nullptr || out[i] == nullptr) return serr("msda_smoother: null pointer");
    if (act_bytes < need_act) return serr("msda_smoother: activation buffer smaller than msda_smoother_workspace_bytes(..., 0)");
    if (!aligned16(act)) return serr("msda_smoother: activation buffer must be 16-byte aligned");
    SmGeo &G = a.G;
    G.act = act;
    for (int i = 0; i < n_calls; ++i) { G.c[i].x = x[i]; G.c[i].out = out[i]; }
    const int per = params_per_module(num_blocks);
    begin_entry();
    const int depths = 2 * num_blocks + 2;
    for (int l = 0; l <= depths; ++l) {                  // l == depths: the fusion
        a.l = l == depths ? sm_fusion_layer(num_blocks) : l;
        a.nprob = 0;
        int tiles = 0;
        for (int m = 0; m < n_mod; ++m)
            for (int s = (l == depths ? 3 : 0); s < (l == depths ? 4 : 3); ++s) {
                SmFwdProb &q = a.p[a.nprob++];
                q.m = m; q.s = s; q.tile0 = tiles;
                q.w = sm_param(params + m * per, num_blocks, s, a.l, 0);
                q.b = sm_param(params + m * per, num_blocks, s, a.l, 1);
                tiles += sm_tiles(G.m[m].rows, sm_layer_n(T, O, H, R, num_blocks, s, a.l));
            }
        if (tiles == 0) continue;
        const bool mid = l >= 1 && l < depths;
        if (mid) hipLaunchKernelGGL(sm_fwd_kernel<true>, dim3((unsigned)tiles), dim3(kHBlock), 0, (hipStream_t)stream, a);
        else hipLaunchKernelGGL(sm_fwd_kernel<false>, dim3((unsigned)tiles), dim3(kHBlock), 0, (hipStream_t)stream, a);
        rc = check_launch("sm_fwd_kernel");
        if (rc != MSDA_OK) return rc;
    }
    return MSDA_OK;
}

int msda_smoother_backward_f32(int T, int O, int H, int R, int num_blocks, int n_mod, int n_calls, const int *call_mod,
                               const int *call_B, const int *call_C, const float *const *x, const float *const *params,
                               const float *act, unsigned long long act_bytes, const float *const *grad_out,
                               float *const *grad_x, float *grad_params, int training, float p,
                               const unsigned long long *seed, void *workspace, unsigned long long workspace_bytes,
                               msda_stream_t stream)
{
    static thread_local SmDgradArgs d;
    static thread_local SmWgradArgs w;
    static thread_local SmFoldArgs f;
    unsigned long long need_act = 0, need_ws = 0;
    int rc = sm_geometry(d.G, T, O, H, R, num_blocks, n_mod, n_calls, call_mod, call_B, call_C, need_act, need_ws);
    if (rc == MSDA_OK) rc = sm_dropout(d.G, training, p, seed);
    if (rc == MSDA_OK) rc = sm_check_params(d.G, params);
    if (rc != MSDA_OK) return rc;
    if (x == nullptr || act == nullptr || grad_out == nullptr || grad_params == nullptr || workspace == nullptr)
        return serr("msda_smoother: null pointer");
    bool want_gx = false;
    for (int i = 0; i < n_calls; ++i) {
        if (x[i] == nullptr || grad_out[i] == nullptr) return serr("msda_smoother: null pointer");
        want_gx = want_gx || (grad_x != nullptr && grad_x[i] != nullptr);
    }
    if (act_bytes < need_act) return serr("msda_smoother: activation buffer smaller than msda_smoother_workspace_bytes(..., 0)");
    if (workspace_bytes < need_ws) return serr("msda_smoother: workspace smaller than msda_smoother_workspace_bytes(..., 1)");
    if (!aligned16(act) || !aligned16(workspace)) return serr("msda_smoother: buffers must be 16-byte aligned");
    SmGeo &G = d.G;
    G.act = const_cast<float *>(act);
    G.ws = static_cast<float *>(workspace);
    G.gp = grad_params;
    for (int i = 0; i < n_calls; ++i) {
        G.c[i].x = x[i];
        G.c[i].gout = grad_out[i];
        G.c[i].gx = grad_x != nullptr ? grad_x[i] : nullptr;
    }
    // the weight-gradient jobs: every layer of every problem
    w.G = G;
    w.njobs = 0;
    int wt = 0;
    const int nl = 2 * num_blocks + 2;
    for (int m = 0; m < n_mod; ++m)
        for (int s = 0; s < 4; ++s)
            for (int l = (s == 3 ? sm_fusion_layer(num_blocks) : 0); l < (s == 3 ? sm_fusion_layer(num_blocks) + 1 : nl); ++l) {
                if (w.njobs == kSmMaxJobs) return serr("msda_smoother: too many layers");
                SmJob &J = w.j[w.njobs++];
                J.tile0 = wt; J.msl = ((m * 4 + s) << 8) | l;
                wt += sm_tiles(sm_layer_n(T, O, H, R, num_blocks, s, l), sm_layer_k(T, O, H, R, num_blocks, s, l));
            }
    f.G = G;
    int fb = 0;
    for (int i = 0; i < n_calls; ++i) {
        f.blk0[i] = fb;
        if (G.c[i].gx != nullptr) fb += (int)(((long long)call_B[i] * T * call_C[i] + kHBlock - 1) / kHBlock);
    }
    f.blk0[n_calls] = fb;
    const int per = params_per_module(num_blocks);
    begin_entry();
    // input gradients: the fusion, the decoders, the blocks top-down, the encoders (only for input gradients)
    for (int step = 0; step <= nl; ++step) {
        const int l = step == 0 ? sm_fusion_layer(num_blocks) : nl - step;     // nl - 1 = decoder ... 0 = encoder
        if (step == nl && !want_gx) break;
        d.l = l;
        d.nprob = 0;
        int tiles = 0;
        for (int m = 0; m < n_mod; ++m)
            for (int s = (step == 0 ? 3 : 0); s < (step == 0 ? 4 : 3); ++s) {
                SmDgradProb &q = d.p[d.nprob++];
                q.m = m; q.s = s; q.tile0 = tiles;
                q.w = sm_param(params + m * per, num_blocks, s, l, 0);
                tiles += sm_tiles(G.m[m].rows, sm_layer_k(T, O, H, R, num_blocks, s, l));
            }
        if (tiles == 0) continue;
        const bool mid = step >= 1 && step < nl;
        if (mid) hipLaunchKernelGGL(sm_dgrad_kernel<true>, dim3((unsigned)tiles), dim3(kHBlock), 0, (hipStream_t)stream, d);
        else hipLaunchKernelGGL(sm_dgrad_kernel<false>, dim3((unsigned)tiles), dim3(kHBlock), 0, (hipStream_t)stream, d);
        rc = check_launch("sm_dgrad_kernel");
        if (rc != MSDA_OK) return rc;
    }
    hipLaunchKernelGGL(sm_wgrad_kernel, dim3((unsigned)wt), dim3(kHBlock), 0, (hipStream_t)stream, w);
    rc = check_launch("sm_wgrad_kernel");
    if (rc != MSDA_OK || fb == 0) return rc;
    hipLaunchKernelGGL(sm_fold_kernel, dim3((unsigned)fb), dim3(kHBlock), 0, (hipStream_t)stream, f);
    return check_launch("sm_fold_kernel");
}

int msda_smoother_dropout_mask_f32(const unsigned long long *seed, int problem, int layer, int rows, int cols, float p, float *mask,
                                   msda_stream_t stream)
{
    if (seed == nullptr || mask == nullptr) return serr("msda_smoother_dropout_mask_f32: null pointer");
    if (problem < 0 || problem >= 1024 || layer < 0 || layer >= 64 || rows < 0 || cols < 0 || rows >= (1 << 24)
        || cols >= (1 << 24) || (long long)rows * cols >= (1LL << 31) || !(p >= 0.f && p < 1.f))
        return serr("msda_smoother_dropout_mask_f32: need problem < 1024, layer < 64, rows, cols < 2^24, 0 <= p < 1");
    const long long n = (long long)rows * cols;
    if (n == 0) return MSDA_OK;
    begin_entry();
    hipLaunchKernelGGL(sm_mask_kernel, dim3((unsigned)((n + kHBlock - 1) / kHBlock)), dim3(kHBlock), 0, (hipStream_t)stream, seed,
                       problem, layer, rows, cols, sm_thresh(p), mask);
    return check_launch("sm_mask_kernel");
}

}  // extern "C"
