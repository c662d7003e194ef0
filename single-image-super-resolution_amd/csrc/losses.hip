// losses.hip -- the two losses of an SRGAN iteration as fused kernels, forward and backward: the feature ("content") MSE of
// train.py:183-186 and the binary cross-entropy of config.py:107.  Nothing here synchronises with the host, nothing uses atomics,
// every sum has a fixed order: the results are the same bits every call and the launches can sit inside a captured step.
//
// Feature MSE, loss = weight * mean((a - b)^2) over n contiguous fp32 elements: a streaming reduction.  The torch expression
// mean(pow(a - b, 2)) moves the tensors through HBM at least 11 times forward + backward and keeps a - b alive; here the forward
// reads a and b once, the backward reads them once more and writes one gradient (5 passes), and nothing is saved.
//   mse_partial_kernel: a capped grid walks tiles of MSE_UNROLL x 256 16-byte loads per operand (all issued before the first
//     use: 32 KB in flight per workgroup), MSE_UNROLL independent 4-lane accumulators per thread, wave shuffles, ONE partial per
//     workgroup into the caller's workspace.
//   mse_finish_kernel: one workgroup adds the partials in a fixed order in double (the metrics_finish_kernel pattern).
//   mse_bwd_kernel: db = c (b - a), da = -db with c = 2 weight g / n, g the upstream gradient read from DEVICE memory.
// Alignment: tensors are only 4-byte aligned in general (a view with an odd storage offset).  When every pointer of a launch
// sits at the same offset inside its 16-byte line, a head of <= 3 elements is peeled so that the body is 16-byte aligned, and
// workgroup 0 takes head and tail one element per thread; otherwise the same kernel runs with one element per load.
//
// BCE, loss = weight * mean(-(t max(log p, -100) + (1 - t) max(log(1 - p), -100))) over a handful of sigmoid outputs (16 per
// D forward): one workgroup, looping for any n; the same launch leaves mean(p) (the D_x / D_G_z statistics the reference fetches
// with .item()).  No range assertion: a NaN or an out-of-range p comes back as a NaN loss.  The clamps are written as comparisons,
// not fmaxf, so that a NaN survives them.  log(1 - p) is evaluated as log1pf(-p): the same function, exact for small p.
#include "sisr_dev.h"

#include <cmath>

#define MSE_UNROLL 4
#define MSE_MAX_WG 2048                        // cdna_hip_programming.md, guideline 11: cap the grid, grid-stride the rest
#define MSE_MAX_N ((int64_t)1 << 40)
#define BCE_GRAD_EPS 1e-12f                    // torch's binary_cross_entropy_backward

__device__ __forceinline__ float lanes_sum(float v) { return v; }
__device__ __forceinline__ float lanes_sum(f32x4 v) { return (v[0] + v[1]) + (v[2] + v[3]); }

// elements of the peeled head: 0..3 so that p + head is 16-byte aligned (p is 4-byte aligned)
static inline int mse_head(const void* p) { return (int)((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) >> 2; }

// grid for `tiles` tiles: capped at MSE_MAX_WG and at SISR_PERSIST_MAX_WG (sisr_cu_slots() is the CU count unless that knob
// lowers it: a lowered value is taken as the workgroup count itself, so that a small input sweeps the grid several times)
static int mse_grid(int64_t tiles) {
    int64_t g = tiles < MSE_MAX_WG ? tiles : MSE_MAX_WG;
    if (const char* e = getenv("SISR_PERSIST_MAX_WG")) {
        if (e[0]) {
            const int slots = sisr_cu_slots();
            if (slots < g) g = slots;
        }
    }
    return g < 1 ? 1 : (int)g;
}

// V = f32x4: a / b point at the 16-byte-aligned body of nv vectors, `head` elements sit before it and `tail` behind it.
// V = float: nv = n, head = tail = 0.  tile = MSE_UNROLL * SISR_BLOCK consecutive V; part[blockIdx.x] = the workgroup's sum.
template <typename V>
__global__ void __launch_bounds__(SISR_BLOCK) mse_partial_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                 int64_t nv, int head, int tail, float* __restrict__ part) {
    constexpr int E = (int)(sizeof(V) / sizeof(float));
    const int tid = threadIdx.x;
    const V* av = reinterpret_cast<const V*>(a);
    const V* bv = reinterpret_cast<const V*>(b);
    const int64_t tile = (int64_t)MSE_UNROLL * SISR_BLOCK;
    V acc[MSE_UNROLL];
#pragma unroll
    for (int u = 0; u < MSE_UNROLL; ++u) acc[u] = V{};
    for (int64_t base = (int64_t)blockIdx.x * tile; base < nv; base += (int64_t)gridDim.x * tile) {
        V x[MSE_UNROLL], y[MSE_UNROLL];
        if (base + tile <= nv) {
#pragma unroll
            for (int u = 0; u < MSE_UNROLL; ++u) { x[u] = av[base + u * SISR_BLOCK + tid]; y[u] = bv[base + u * SISR_BLOCK + tid]; }
        } else {
#pragma unroll
            for (int u = 0; u < MSE_UNROLL; ++u) {
                const int64_t i = base + u * SISR_BLOCK + tid;
                x[u] = V{}; y[u] = V{};
                if (i < nv) { x[u] = av[i]; y[u] = bv[i]; }
            }
        }
#pragma unroll
        for (int u = 0; u < MSE_UNROLL; ++u) { const V d = x[u] - y[u]; acc[u] += d * d; }
    }
    float s[1] = {lanes_sum((acc[0] + acc[1]) + (acc[2] + acc[3]))};
    static_assert(MSE_UNROLL == 4, "the accumulators are folded pairwise above");
    if (blockIdx.x == 0) {                     // the <= 3 + 3 elements around the aligned body
        if (tid < head) { const float d = a[tid - head] - b[tid - head]; s[0] += d * d; }
        if (tid < tail) { const float d = a[nv * E + tid] - b[nv * E + tid]; s[0] += d * d; }
    }
    block_partial_sum(s);
    if (tid == 0) part[blockIdx.x] = s[0];
}

// one workgroup: the partials added in a fixed order in double (fold_partials_double); out = weight * sum / n
__global__ void __launch_bounds__(SISR_BLOCK) mse_finish_kernel(const float* __restrict__ part, int count, double n, float weight,
                                                                float* __restrict__ out) {
    double s[1];
    fold_partials_double(count, s, [&](int64_t i, double* acc) { acc[0] += (double)part[i]; });
    if (threadIdx.x == 0) out[0] = (float)((double)weight * s[0] / n);
}

// same tiling as the forward; da / db: either may be null.  c is formed in double from the fp32 weight and the fp32 upstream
// gradient and rounded once, so an element carries three fp32 roundings (c, b - a, the product)
template <typename V>
__global__ void __launch_bounds__(SISR_BLOCK) mse_bwd_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                             const float* __restrict__ g, float weight, double n, int64_t nv,
                                                             int head, int tail, float* __restrict__ da, float* __restrict__ db) {
    constexpr int E = (int)(sizeof(V) / sizeof(float));
    const int tid = threadIdx.x;
    const float c = (float)(2.0 * (double)weight * (double)g[0] / n);
    const V* av = reinterpret_cast<const V*>(a);
    const V* bv = reinterpret_cast<const V*>(b);
    V* dav = reinterpret_cast<V*>(da);
    V* dbv = reinterpret_cast<V*>(db);
    const int64_t tile = (int64_t)MSE_UNROLL * SISR_BLOCK;
    for (int64_t base = (int64_t)blockIdx.x * tile; base < nv; base += (int64_t)gridDim.x * tile) {
        V x[MSE_UNROLL], y[MSE_UNROLL];
        const bool full = base + tile <= nv;
#pragma unroll
        for (int u = 0; u < MSE_UNROLL; ++u) {
            const int64_t i = base + u * SISR_BLOCK + tid;
            x[u] = V{}; y[u] = V{};
            if (full || i < nv) { x[u] = av[i]; y[u] = bv[i]; }
        }
#pragma unroll
        for (int u = 0; u < MSE_UNROLL; ++u) {
            const int64_t i = base + u * SISR_BLOCK + tid;
            const V r = c * (y[u] - x[u]);
            if (full || i < nv) {
                if (db) dbv[i] = r;
                if (da) dav[i] = -r;
            }
        }
    }
    if (blockIdx.x == 0) {
        if (tid < head) {
            const float r = c * (b[tid - head] - a[tid - head]);
            if (db) db[tid - head] = r;
            if (da) da[tid - head] = -r;
        }
        if (tid < tail) {
            const int64_t i = nv * E + tid;
            const float r = c * (b[i] - a[i]);
            if (db) db[i] = r;
            if (da) da[i] = -r;
        }
    }
}

// one workgroup; tv: n targets, or null for the scalar ts.  loss / mean_p: either may be null
__global__ void __launch_bounds__(SISR_BLOCK) bce_fwd_kernel(const float* __restrict__ p, const float* __restrict__ tv, float ts,
                                                             int64_t n, float weight, float* __restrict__ loss,
                                                             float* __restrict__ mean_p) {
    double s[2];          // sum of the losses, sum of p
    fold_partials_double(n, s, [&](int64_t i, double* acc) {
        const float v = p[i], t = tv ? tv[i] : ts;
        float l1 = logf(v), l0 = log1pf(-v);
        l1 = l1 < -100.f ? -100.f : l1;        // (not fmaxf: a NaN must stay a NaN)
        l0 = l0 < -100.f ? -100.f : l0;
        acc[0] += (double)(-(t * l1 + (1.f - t) * l0));
        acc[1] += (double)v;
    });
    if (threadIdx.x == 0) {
        if (loss) loss[0] = (float)((double)weight * s[0] / (double)n);
        if (mean_p) mean_p[0] = (float)(s[1] / (double)n);
    }
}

// dp = weight g (p - t) / max(p (1 - p), 1e-12) / n
__global__ void __launch_bounds__(SISR_BLOCK) bce_bwd_kernel(const float* __restrict__ p, const float* __restrict__ tv, float ts,
                                                             int64_t n, float weight, const float* __restrict__ g,
                                                             float* __restrict__ dp) {
    const float c = (float)((double)weight * (double)g[0] / (double)n);
    for (int64_t i = (int64_t)blockIdx.x * SISR_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * SISR_BLOCK) {
        const float v = p[i], t = tv ? tv[i] : ts;
        float d = v * (1.f - v);
        d = d < BCE_GRAD_EPS ? BCE_GRAD_EPS : d;
        dp[i] = c * ((v - t) / d);
    }
}

extern "C" int sisr_mse_ws_floats(int64_t n) {
    if (n < 1) return SISR_E_BADARG;
    if (n > MSE_MAX_N) return SISR_E_TOOBIG;
    return MSE_MAX_WG;                         // one partial per workgroup of the largest grid, whatever the knobs say later
}

// the common split of a launch: vector body when every pointer shares its offset inside a 16-byte line
struct MseSplit { bool vec; int head, tail; int64_t nv, tiles; };
static MseSplit mse_split(int64_t n, const void* p0, const void* p1, const void* p2, const void* p3) {
    MseSplit s;
    const int h = mse_head(p0);
    s.vec = h == mse_head(p1) && (!p2 || h == mse_head(p2)) && (!p3 || h == mse_head(p3));
    if (s.vec) {
        s.head = (int64_t)h < n ? h : (int)n;
        s.nv = (n - s.head) >> 2;
        s.tail = (int)(n - s.head - 4 * s.nv);
    } else {
        s.head = 0; s.tail = 0; s.nv = n;
    }
    const int64_t tile = (int64_t)MSE_UNROLL * SISR_BLOCK;
    s.tiles = (s.nv + tile - 1) / tile;
    return s;
}

extern "C" int sisr_mse_fwd(const float* a, const float* b, int64_t n, float weight, float* work, float* loss, void* stream) {
    const int ws = sisr_mse_ws_floats(n);
    if (ws < 0) return ws;
    if (!a || !b || !work || !loss || (((uintptr_t)a | (uintptr_t)b) & 3u)) return SISR_E_BADARG;
    const MseSplit s = mse_split(n, a, b, nullptr, nullptr);
    const int grid = mse_grid(s.tiles);
    hipStream_t st = sisr_stream(stream);
    if (s.vec)
        hipLaunchKernelGGL(mse_partial_kernel<f32x4>, dim3((unsigned)grid), dim3(SISR_BLOCK), 0, st, a + s.head, b + s.head, s.nv,
                           s.head, s.tail, work);
    else
        hipLaunchKernelGGL(mse_partial_kernel<float>, dim3((unsigned)grid), dim3(SISR_BLOCK), 0, st, a, b, s.nv, 0, 0, work);
    SISR_CHECK_LAUNCH();
    hipLaunchKernelGGL(mse_finish_kernel, dim3(1), dim3(SISR_BLOCK), 0, st, (const float*)work, grid, (double)n, weight, loss);
    SISR_CHECK_LAUNCH();
    return 0;
}

extern "C" int sisr_mse_bwd(const float* a, const float* b, const float* g, int64_t n, float weight, float* da, float* db,
                            void* stream) {
    if (n < 1) return SISR_E_BADARG;
    if (n > MSE_MAX_N) return SISR_E_TOOBIG;
    if (!a || !b || !g || (!da && !db)) return SISR_E_BADARG;
    if (((uintptr_t)a | (uintptr_t)b | (uintptr_t)da | (uintptr_t)db) & 3u) return SISR_E_BADARG;
    const MseSplit s = mse_split(n, a, b, da, db);
    const int grid = mse_grid(s.tiles);
    hipStream_t st = sisr_stream(stream);
    if (s.vec)
        hipLaunchKernelGGL(mse_bwd_kernel<f32x4>, dim3((unsigned)grid), dim3(SISR_BLOCK), 0, st, a + s.head, b + s.head, g, weight,
                           (double)n, s.nv, s.head, s.tail, da ? da + s.head : nullptr, db ? db + s.head : nullptr);
    else
        hipLaunchKernelGGL(mse_bwd_kernel<float>, dim3((unsigned)grid), dim3(SISR_BLOCK), 0, st, a, b, g, weight, (double)n, s.nv,
                           0, 0, da, db);
    SISR_CHECK_LAUNCH();
    return 0;
}

extern "C" int sisr_bce_fwd(const float* p, const float* t_vec, float t_scalar, int64_t n, float weight, float* loss,
                            float* mean_p, void* stream) {
    if (n < 1 || !p || (!loss && !mean_p)) return SISR_E_BADARG;
    hipLaunchKernelGGL(bce_fwd_kernel, dim3(1), dim3(SISR_BLOCK), 0, sisr_stream(stream), p, t_vec, t_scalar, n, weight, loss,
                       mean_p);
    SISR_CHECK_LAUNCH();
    return 0;
}

extern "C" int sisr_bce_bwd(const float* p, const float* t_vec, float t_scalar, int64_t n, float weight, const float* g,
                            float* dp, void* stream) {
    if (n < 1 || !p || !g || !dp) return SISR_E_BADARG;
    const int64_t blocks = (n + SISR_BLOCK - 1) / SISR_BLOCK;
    hipLaunchKernelGGL(bce_bwd_kernel, dim3((unsigned)mse_grid(blocks)), dim3(SISR_BLOCK), 0, sisr_stream(stream), p, t_vec,
                       t_scalar, n, weight, g, dp);
    SISR_CHECK_LAUNCH();
    return 0;
}
