// optim.hip -- fused multi-tensor Adam step: one launch updates every parameter of a network.
// Replaces the per-step optimizer passes of the reference, torch.optim.Adam(net.parameters(), lr, betas=(.9, .999))
// (config.py:292-294; stepped at train.py:75,108), with torch's semantics for amsgrad=False, maximize=False:
//     g' = g + wd * p ;  m = m + (g' - m) * (1 - b1) ;  v = v * b2 + (1 - b2) * g'^2
//     p -= (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// HBM-bound: 4 reads + 3 writes of 4 bytes per parameter.  The descriptor table lives in device memory; a workgroup
// finds its tensor by a binary search over the per-tensor first-block indices.
//
// Two families share the update (AdamUpdate):
//   host state    adam_step_kernel: lr and the bias corrections arrive as launch arguments (sisr_adam_step);
//   device state  the step count of every tensor, the learning rate and the guards live in device memory, so the launches
//                 below can sit inside a captured HIP graph and still advance from replay to replay:
//       adam_sumsq_kernel    (guards only) one double partial of sum g^2 per workgroup, same block mapping as the step;
//       adam_prepare_kernel  one thread per tensor: partials -> norm / clip coefficient / skip flag, t -> t + 1, and the
//                            tensor's step_size and 1 / sqrt(1 - beta2^t);
//       adam_step_dev_kernel the update with those per-tensor constants, g scaled by the clip coefficient, nothing stored
//                            when the skip flag is set.
// No atomics, every sum in a fixed order: the same inputs give the same bits.
//
// The weight EMA is the same kind of kernel on the same block mapping, over SisrEmaDesc tables:
//       ema_prepare_kernel   one thread: update count -> decay of this update -> control block { 1 - d, active }, count + 1;
//       ema_update_kernel    shadow += (1 - d) * (live - shadow) (mode 0) or shadow = live (mode 1), nothing when not active;
//       ema_swap_kernel      exchanges the bits of shadow and live tensor.
#include "sisr_dev.h"

#include <cmath>

#define ADAM_CHUNK (SISR_BLOCK * 16)          // elements per workgroup

// control block of the device-state family: four 32-bit words
#define ADAM_CTRL_NORM 0                      // fp32  global gradient norm of the last guarded step
#define ADAM_CTRL_COEF 1                      // fp32  min(1, max_norm / (norm + 1e-6))
#define ADAM_CTRL_SKIP 2                      // int32 1: the last step was skipped (non-finite norm)
#define ADAM_CTRL_SKIPPED 3                   // int32 running count of skipped steps

// index of the last tensor whose block_start <= block (SisrAdamDesc or SisrEmaDesc: the same block mapping)
template <typename Desc>
__device__ __forceinline__ int adam_find_tensor(const Desc* __restrict__ table, int n, int64_t block) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].block_start <= block) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// THE block mapping: workgroup blockIdx.x owns ADAM_CHUNK elements of table row `row` (copied to t), starting at element `base`
template <typename Desc> struct Chunk { int row; Desc t; int64_t base; };
template <typename Desc> __device__ __forceinline__ Chunk<Desc> chunk_of_block(const Desc* __restrict__ table, int n) {
    const int row = adam_find_tensor(table, n, (int64_t)blockIdx.x);
    const Desc t = table[row];
    return {row, t, ((int64_t)blockIdx.x - t.block_start) * ADAM_CHUNK};
}

// THE rule of the 16-byte path: whole 16-byte items only, and every tensor the kernel touches starts on a 16-byte line (a
// parameter or a gradient may be a view at an odd element offset); everything else takes the 4-byte path
template <typename... P>
__device__ __forceinline__ bool chunk_vec_ok(int64_t numel, const P*... ptrs) {
    return ((numel & 3) | ((... | reinterpret_cast<uintptr_t>(ptrs)) & 15)) == 0;
}

template <int W> using fvec = float __attribute__((ext_vector_type(W)));
template <int W> using uvec = unsigned __attribute__((ext_vector_type(W)));

// THE walk over a chunk, in items of W elements (4: the 16-byte path, 4 items per thread; 1: 16 items per thread) at stride
// SISR_BLOCK.  Op: Item<W> = what a thread holds of one item, load<W>(i, item), apply<W>(i, item) = arithmetic and stores.  A thread
// issues the loads of G items before the first of them is applied; G == 1 loads and applies an item under ONE bounds test (with
// two, loads stay pending across a branch and the compiler's wait counting then waits between the 16-byte loads of the Adam step)
template <int W, int G, typename Op>
__device__ __forceinline__ void chunk_walk_items(int64_t numel, int64_t base, Op& op) {
    constexpr int SHIFT = W == 4 ? 2 : 0, UNROLL = W == 4 ? 4 : 1;          // (the 4-byte path stays a loop)
    const int64_t ni = numel >> SHIFT, i0 = (base >> SHIFT) + threadIdx.x;
#pragma unroll UNROLL
    for (int k = 0; k < 16 / W; k += G) {
        typename Op::template Item<W> x[G];
#pragma unroll
        for (int u = 0; u < G; ++u) {
            const int64_t i = i0 + (k + u) * SISR_BLOCK;
            if (i < ni) {
                op.template load<W>(i, x[u]);
                if (G == 1) op.template apply<W>(i, x[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < G; ++u) {
            const int64_t i = i0 + (k + u) * SISR_BLOCK;
            if (G > 1 && i < ni) op.template apply<W>(i, x[u]);
        }
    }
}
template <int G, typename Op>
__device__ __forceinline__ void chunk_walk(bool vec, int64_t numel, int64_t base, Op& op) {
    if (vec) chunk_walk_items<4, G>(numel, base, op); else chunk_walk_items<1, G>(numel, base, op);
}

// a * b + c * d.  Written as that sum, the compiler may fuse either product into the addition or neither, and its pick moves with
// the code around the line (it differed between the two loops of one kernel).  A resumed run must keep its bits, so the update's
// two such sums say which product is fused (FUSE 1: a * b, 2: c * d, 0: none; the other is rounded first): what each path always did
template <int FUSE>
__device__ __forceinline__ float sum_of_products(float a, float b, float c, float d) {
#pragma clang fp contract(off)
    const float ab = a * b, cd = c * d;
    return FUSE == 1 ? fmaf(a, b, cd) : FUSE == 2 ? fmaf(c, d, ab) : ab + cd;
}

// the Adam update.  CLIP: g is multiplied by coef before the weight decay is added (the gradient tensor itself is only read)
template <bool CLIP>
struct AdamUpdate {
    const SisrAdamDesc& t;
    float coef, step_size, omb1, beta2, omb2, eps, wd, inv_sqrt_bc2;
    template <int W> struct Item { fvec<W> p, g, m, v; };
    template <int W> __device__ __forceinline__ void load(int64_t i, Item<W>& x) const {
        x.p = reinterpret_cast<const fvec<W>*>(t.p)[i]; x.g = reinterpret_cast<const fvec<W>*>(t.g)[i];
        x.m = reinterpret_cast<const fvec<W>*>(t.m)[i]; x.v = reinterpret_cast<const fvec<W>*>(t.v)[i];
    }
    template <int W> __device__ __forceinline__ void apply(int64_t i, Item<W>& x) const {
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const float gg = CLIP ? sum_of_products<W == 4 ? 2 : 1>(x.g[j], coef, wd, x.p[j]) : x.g[j] + wd * x.p[j];
            x.m[j] = x.m[j] + (gg - x.m[j]) * omb1;
            x.v[j] = sum_of_products<W == 4 ? 1 : 0>(x.v[j], beta2, omb2 * gg, gg);
            x.p[j] -= step_size * (x.m[j] / (sqrtf(x.v[j]) * inv_sqrt_bc2 + eps));
        }
        reinterpret_cast<fvec<W>*>(t.p)[i] = x.p; reinterpret_cast<fvec<W>*>(t.m)[i] = x.m; reinterpret_cast<fvec<W>*>(t.v)[i] = x.v;
    }
};
template <bool CLIP>
__device__ __forceinline__ void adam_update_chunk(const Chunk<SisrAdamDesc>& c, AdamUpdate<CLIP> op) {
    chunk_walk<1>(chunk_vec_ok(c.t.numel, c.t.p, c.t.m, c.t.v, c.t.g), c.t.numel, c.base, op);          // item by item
}

__global__ void __launch_bounds__(SISR_BLOCK) adam_step_kernel(const SisrAdamDesc* __restrict__ table, int n, float step_size,
                                                                float omb1, float beta2, float omb2, float eps, float wd,
                                                                float inv_sqrt_bc2) {
    const Chunk<SisrAdamDesc> c = chunk_of_block(table, n);
    adam_update_chunk<false>(c, {c.t, 1.f, step_size, omb1, beta2, omb2, eps, wd, inv_sqrt_bc2});
}

// ---- device-state family ------------------------------------------------------------------------------------------------

struct GradSumsq {
    const float* g;
    double s[1];
    template <int W> struct Item { fvec<W> g; };
    template <int W> __device__ __forceinline__ void load(int64_t i, Item<W>& x) const { x.g = reinterpret_cast<const fvec<W>*>(g)[i]; }
    template <int W> __device__ __forceinline__ void apply(int64_t, Item<W>& x) {
#pragma unroll
        for (int j = 0; j < W; ++j) s[0] += (double)x.g[j] * (double)x.g[j];
    }
};

// part[blockIdx.x] = sum of g^2 over the workgroup's chunk, squared and accumulated in double (|g| ~ 1e19 overflows an fp32
// square; the kernel waits for HBM either way): per thread in item order, then block_partial_sum
__global__ void __launch_bounds__(SISR_BLOCK) adam_sumsq_kernel(const SisrAdamDesc* __restrict__ table, int n,
                                                                 double* __restrict__ part) {
    const Chunk<SisrAdamDesc> c = chunk_of_block(table, n);
    GradSumsq op = {c.t.g, {0.0}};
    chunk_walk<4>(chunk_vec_ok(c.t.numel, c.t.g), c.t.numel, c.base, op);
    block_partial_sum(op.s);
    if (threadIdx.x == 0) part[blockIdx.x] = op.s[0];
}

// One thread per tensor, ceil(n / 256) workgroups.  With partials (n_part > 0) EVERY workgroup adds all of them in the same
// fixed order in double (thread t takes t, t + 256, ...; pairwise fold through LDS), so each one holds the same norm bits and
// no workgroup waits for another; workgroup 0 stores the control block when write_ctrl is set.  max_norm < 0: no clipping.
// Then per tensor: t = *steps[i]; step_size = lr / (1 - beta1^(t+1)) and 1 / sqrt(1 - beta2^(t+1)) in double, rounded to fp32
// once (the rule of sisr_adam_step); *steps[i] = t + 1.  A skipped step stores neither.
__global__ void __launch_bounds__(SISR_BLOCK) adam_prepare_kernel(float* const* __restrict__ steps, int n, const void* __restrict__ lr,
                                                                   int lr_f64, double beta1, double beta2,
                                                                   const double* __restrict__ part, int64_t n_part, double max_norm,
                                                                   int skip_nonfinite, int write_ctrl, float* __restrict__ ctrl,
                                                                   float* __restrict__ consts) {
    const int tid = threadIdx.x;
    float norm_f = 0.f, coef = 1.f;
    int skip = 0;
    if (n_part > 0) {
        double s[1];
        fold_partials_double(n_part, s, [&](int64_t i, double* a) { a[0] += part[i]; });
        const double norm = sqrt(s[0]);
        norm_f = (float)norm;
        if (max_norm >= 0.0) {
            const double c = max_norm / (norm + 1e-6);          // torch.nn.utils.clip_grad_norm_
            coef = !(c >= 1.0) ? (float)c : 1.f;                // (a NaN norm stays a NaN coefficient, as torch's clamp leaves it)
        }
        skip = skip_nonfinite && !isfinite(norm_f);
    }
    if (write_ctrl && blockIdx.x == 0 && tid == 0) {
        int* ictrl = reinterpret_cast<int*>(ctrl);
        ctrl[ADAM_CTRL_NORM] = norm_f;
        ctrl[ADAM_CTRL_COEF] = coef;
        ictrl[ADAM_CTRL_SKIP] = skip;
        ictrl[ADAM_CTRL_SKIPPED] += skip;
    }
    const int i = blockIdx.x * SISR_BLOCK + tid;
    if (i < n && !skip) {
        const double t1 = (double)steps[i][0] + 1.0;
        const double lr_now = lr_f64 ? *reinterpret_cast<const double*>(lr) : (double)*reinterpret_cast<const float*>(lr);
        consts[2 * i] = (float)(lr_now / (1.0 - pow(beta1, t1)));
        consts[2 * i + 1] = (float)(1.0 / sqrt(1.0 - pow(beta2, t1)));
        steps[i][0] = (float)t1;
    }
}

__global__ void __launch_bounds__(SISR_BLOCK) adam_step_dev_kernel(const SisrAdamDesc* __restrict__ table, int n,
                                                                    const float* __restrict__ consts, const float* __restrict__ ctrl,
                                                                    float omb1, float beta2, float omb2, float eps, float wd) {
    if (reinterpret_cast<const int*>(ctrl)[ADAM_CTRL_SKIP]) return;          // before any store
    const Chunk<SisrAdamDesc> c = chunk_of_block(table, n);
    adam_update_chunk<true>(c, {c.t, ctrl[ADAM_CTRL_COEF], consts[2 * c.row], omb1, beta2, omb2, eps, wd, consts[2 * c.row + 1]});
}

extern "C" int64_t sisr_adam_blocks(int64_t numel) { return numel <= 0 ? 0 : (numel + ADAM_CHUNK - 1) / ADAM_CHUNK; }

extern "C" int sisr_adam_step(const SisrAdamDesc* table_dev, int32_t n, int64_t total_blocks, double lr, double beta1,
                              double beta2, double eps, double weight_decay, double bias_corr1, double bias_corr2,
                              void* stream) {
    if (!table_dev || n <= 0 || total_blocks <= 0 || total_blocks >= (1ll << 31) || bias_corr1 <= 0.0 || bias_corr2 <= 0.0)
        return SISR_E_BADARG;
    // host scalars are doubles (as in torch): 1 - beta, lr / bias_corr1 ... are rounded to fp32 once, after the arithmetic
    hipLaunchKernelGGL(adam_step_kernel, dim3((unsigned)total_blocks), dim3(SISR_BLOCK), 0, sisr_stream(stream),
                       table_dev, n, (float)(lr / bias_corr1), (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2),
                       (float)eps, (float)weight_decay, (float)(1.0 / sqrt(bias_corr2)));
    SISR_CHECK_LAUNCH();
    return 0;
}

static inline bool adam_blocks_ok(int64_t total_blocks) { return total_blocks > 0 && total_blocks < (1ll << 31); }
static inline bool adam_beta_ok(double b) { return b >= 0.0 && b < 1.0; }          // (false for a NaN)

extern "C" int64_t sisr_adam_norm_ws_doubles(int64_t total_blocks) {
    return adam_blocks_ok(total_blocks) ? total_blocks : (int64_t)SISR_E_BADARG;
}

extern "C" int sisr_adam_grad_sumsq(const SisrAdamDesc* table_dev, int32_t n, int64_t total_blocks, double* partials, void* stream) {
    if (!table_dev || n <= 0 || !adam_blocks_ok(total_blocks) || !partials) return SISR_E_BADARG;
    hipLaunchKernelGGL(adam_sumsq_kernel, dim3((unsigned)total_blocks), dim3(SISR_BLOCK), 0, sisr_stream(stream), table_dev, n,
                       partials);
    SISR_CHECK_LAUNCH();
    return 0;
}

extern "C" int sisr_adam_prepare(float* const* steps_dev, int32_t n, const void* lr_dev, int32_t lr_is_f64, double beta1, double beta2,
                                 const double* partials, int64_t n_partials, double max_norm, int32_t skip_nonfinite,
                                 int32_t write_ctrl, float* ctrl, float* consts, void* stream) {
    if (!steps_dev || n <= 0 || !lr_dev || !ctrl || !consts || !adam_beta_ok(beta1) || !adam_beta_ok(beta2)) return SISR_E_BADARG;
    if (n_partials < 0 || n_partials >= (1ll << 31) || (n_partials > 0 && !partials) || max_norm != max_norm) return SISR_E_BADARG;
    hipLaunchKernelGGL(adam_prepare_kernel, dim3((unsigned)((n + SISR_BLOCK - 1) / SISR_BLOCK)), dim3(SISR_BLOCK), 0,
                       sisr_stream(stream), steps_dev, n, lr_dev, lr_is_f64, beta1, beta2, partials, n_partials, max_norm,
                       skip_nonfinite, write_ctrl, ctrl, consts);
    SISR_CHECK_LAUNCH();
    return 0;
}

extern "C" int sisr_adam_step_dev(const SisrAdamDesc* table_dev, int32_t n, int64_t total_blocks, const float* consts,
                                  const float* ctrl, double beta1, double beta2, double eps, double weight_decay, void* stream) {
    if (!table_dev || n <= 0 || !adam_blocks_ok(total_blocks) || !consts || !ctrl || !adam_beta_ok(beta1) || !adam_beta_ok(beta2))
        return SISR_E_BADARG;
    hipLaunchKernelGGL(adam_step_dev_kernel, dim3((unsigned)total_blocks), dim3(SISR_BLOCK), 0, sisr_stream(stream), table_dev, n,
                       consts, ctrl, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps, (float)weight_decay);
    SISR_CHECK_LAUNCH();
    return 0;
}

// ---- weight EMA ------------------------------------------------------------------------------------

// control block of the EMA launches: two 32-bit words, written only by ema_prepare_kernel
#define EMA_CTRL_OMD 0                        // fp32  1 - decay of this update
#define EMA_CTRL_ACTIVE 1                     // int32 0: the followed optimizer skipped its step, the update stores nothing

// an element whose live value equals its average keeps its bits (e + omd * 0 would turn a -0 into +0)
__device__ __forceinline__ float ema_value(float e, float p, float omd) {
    const float d = p - e;
    return d == 0.f ? e : e + omd * d;
}

// One thread; the only code that reads or writes the update count.  d = min(decay, (1 + n) / (warmup + n)) (warmup > 0) in
// double, 1 - d rounded to fp32 once.  With a skip flag that is set: active = 0, count and 1 - d stay.
__global__ void __launch_bounds__(64) ema_prepare_kernel(int* __restrict__ count, double decay, double warmup,
                                                          const int* __restrict__ skip_flag, float* __restrict__ ctrl) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    int* ictrl = reinterpret_cast<int*>(ctrl);
    if (skip_flag && *skip_flag != 0) { ictrl[EMA_CTRL_ACTIVE] = 0; return; }
    const int n = *count;
    double d = decay;
    if (warmup > 0.0) d = fmin(decay, (1.0 + (double)n) / (warmup + (double)n));
    ctrl[EMA_CTRL_OMD] = (float)(1.0 - d);
    ictrl[EMA_CTRL_ACTIVE] = 1;
    *count = n + 1;
}

// the three per-item bodies: average, bit copy live -> shadow, bit exchange
struct EmaAverage {
    const SisrEmaDesc& t;
    float omd;
    template <int W> struct Item { fvec<W> e, p; };
    template <int W> __device__ __forceinline__ void load(int64_t i, Item<W>& x) const {
        x.e = reinterpret_cast<const fvec<W>*>(t.ema)[i]; x.p = reinterpret_cast<const fvec<W>*>(t.src)[i];
    }
    template <int W> __device__ __forceinline__ void apply(int64_t i, Item<W>& x) const {
#pragma unroll
        for (int j = 0; j < W; ++j) x.e[j] = ema_value(x.e[j], x.p[j], omd);
        reinterpret_cast<fvec<W>*>(t.ema)[i] = x.e;
    }
};
template <bool SWAP>
struct EmaBits {
    const SisrEmaDesc& t;
    template <int W> struct Item { uvec<W> e, p; };
    template <int W> __device__ __forceinline__ void load(int64_t i, Item<W>& x) const {
        if (SWAP) x.e = reinterpret_cast<const uvec<W>*>(t.ema)[i];
        x.p = reinterpret_cast<const uvec<W>*>(t.src)[i];
    }
    template <int W> __device__ __forceinline__ void apply(int64_t i, Item<W>& x) const {
        reinterpret_cast<uvec<W>*>(t.ema)[i] = x.p;
        if (SWAP) reinterpret_cast<uvec<W>*>(t.src)[i] = x.e;
    }
};
// all loads of a thread's four 16-byte items are issued before its first store
template <typename Op>
__device__ __forceinline__ void ema_walk(const Chunk<SisrEmaDesc>& c, Op op) {
    chunk_walk<4>(chunk_vec_ok(c.t.numel, c.t.ema, c.t.src), c.t.numel, c.base, op);
}

__global__ void __launch_bounds__(SISR_BLOCK) ema_update_kernel(const SisrEmaDesc* __restrict__ table, int n,
                                                                 const float* __restrict__ ctrl) {
    if (reinterpret_cast<const int*>(ctrl)[EMA_CTRL_ACTIVE] == 0) return;          // before any store
    const Chunk<SisrEmaDesc> c = chunk_of_block(table, n);
    if (c.t.mode == 0) ema_walk(c, EmaAverage{c.t, ctrl[EMA_CTRL_OMD]}); else ema_walk(c, EmaBits<false>{c.t});
}

__global__ void __launch_bounds__(SISR_BLOCK) ema_swap_kernel(const SisrEmaDesc* __restrict__ table, int n) {
    const Chunk<SisrEmaDesc> c = chunk_of_block(table, n);
    ema_walk(c, EmaBits<true>{c.t});
}

extern "C" int sisr_ema_prepare(int32_t* count_dev, double decay, double warmup, const int32_t* skip_flag_dev, float* ctrl,
                                void* stream) {
    if (!count_dev || !ctrl || !adam_beta_ok(decay) || !(warmup >= 0.0)) return SISR_E_BADARG;          // (false for a NaN)
    hipLaunchKernelGGL(ema_prepare_kernel, dim3(1), dim3(64), 0, sisr_stream(stream), count_dev, decay, warmup, skip_flag_dev, ctrl);
    SISR_CHECK_LAUNCH();
    return 0;
}

extern "C" int sisr_ema_update(const SisrEmaDesc* table_dev, int32_t n, int64_t total_blocks, const float* ctrl, void* stream) {
    if (!table_dev || n <= 0 || !adam_blocks_ok(total_blocks) || !ctrl) return SISR_E_BADARG;
    hipLaunchKernelGGL(ema_update_kernel, dim3((unsigned)total_blocks), dim3(SISR_BLOCK), 0, sisr_stream(stream), table_dev, n, ctrl);
    SISR_CHECK_LAUNCH();
    return 0;
}

extern "C" int sisr_ema_swap(const SisrEmaDesc* table_dev, int32_t n, int64_t total_blocks, void* stream) {
    if (!table_dev || n <= 0 || !adam_blocks_ok(total_blocks)) return SISR_E_BADARG;
    hipLaunchKernelGGL(ema_swap_kernel, dim3((unsigned)total_blocks), dim3(SISR_BLOCK), 0, sisr_stream(stream), table_dev, n);
    SISR_CHECK_LAUNCH();
    return 0;
}
