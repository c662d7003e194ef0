// optim.hip -- fused multi-tensor Adam step: one launch updates every parameter of a network.
// Replaces the per-step optimizer passes of the reference, torch.optim.Adam(net.parameters(), lr, betas=(.9, .999))
// (config.py:292-294; stepped at train.py:75,108), with torch's semantics for amsgrad=False, maximize=False:
//     g' = g + wd * p ;  m = m + (g' - m) * (1 - b1) ;  v = v * b2 + (1 - b2) * g'^2
//     p -= (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// HBM-bound: 4 reads + 3 writes of 4 bytes per parameter.  The descriptor table lives in device memory; a workgroup
// finds its tensor by a binary search over the per-tensor first-block indices.
//
// Two families share the update (adam_update_block):
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

// the update of one workgroup's ADAM_CHUNK elements of tensor t, starting at element `base`.  CLIP: g is multiplied by coef
// before the weight decay is added (the gradient tensor itself is only read)
template <bool CLIP>
__device__ __forceinline__ void adam_update_block(const SisrAdamDesc& t, int64_t base, float coef, float step_size, float omb1,
                                                  float beta2, float omb2, float eps, float wd, float inv_sqrt_bc2) {
    if ((t.numel & 3) == 0) {
        const int64_t n4 = t.numel >> 2;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t i = (base >> 2) + k * SISR_BLOCK + threadIdx.x;
            if (i < n4) {
                f32x4 p = reinterpret_cast<const f32x4*>(t.p)[i], g = reinterpret_cast<const f32x4*>(t.g)[i];
                f32x4 m = reinterpret_cast<const f32x4*>(t.m)[i], v = reinterpret_cast<const f32x4*>(t.v)[i];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float gg = (CLIP ? g[j] * coef : g[j]) + wd * p[j];
                    m[j] = m[j] + (gg - m[j]) * omb1;
                    v[j] = v[j] * beta2 + omb2 * gg * gg;
                    p[j] -= step_size * (m[j] / (sqrtf(v[j]) * inv_sqrt_bc2 + eps));
                }
                reinterpret_cast<f32x4*>(t.p)[i] = p;
                reinterpret_cast<f32x4*>(t.m)[i] = m;
                reinterpret_cast<f32x4*>(t.v)[i] = v;
            }
        }
    } else {
        for (int k = 0; k < 16; ++k) {
            const int64_t i = base + k * SISR_BLOCK + threadIdx.x;
            if (i < t.numel) {
                const float gg = (CLIP ? t.g[i] * coef : t.g[i]) + wd * t.p[i];
                const float m = t.m[i] + (gg - t.m[i]) * omb1;
                const float v = t.v[i] * beta2 + omb2 * gg * gg;
                t.m[i] = m; t.v[i] = v;
                t.p[i] -= step_size * (m / (sqrtf(v) * inv_sqrt_bc2 + eps));
            }
        }
    }
}

__global__ void __launch_bounds__(SISR_BLOCK) adam_step_kernel(const SisrAdamDesc* __restrict__ table, int n, float step_size,
                                                                float omb1, float beta2, float omb2, float eps, float wd,
                                                                float inv_sqrt_bc2) {
    const SisrAdamDesc t = table[adam_find_tensor(table, n, (int64_t)blockIdx.x)];
    const int64_t base = ((int64_t)blockIdx.x - t.block_start) * ADAM_CHUNK;
    adam_update_block<false>(t, base, 1.f, step_size, omb1, beta2, omb2, eps, wd, inv_sqrt_bc2);
}

// ---- device-state family ------------------------------------------------------------------------------------------------

// part[blockIdx.x] = sum of g^2 over the workgroup's chunk, squared and accumulated in double (|g| ~ 1e19 overflows an fp32
// square; the kernel waits for HBM either way)
__global__ void __launch_bounds__(SISR_BLOCK) adam_sumsq_kernel(const SisrAdamDesc* __restrict__ table, int n,
                                                                 double* __restrict__ part) {
    __shared__ double red[SISR_BLOCK / 64];
    const SisrAdamDesc t = table[adam_find_tensor(table, n, (int64_t)blockIdx.x)];
    const int64_t base = ((int64_t)blockIdx.x - t.block_start) * ADAM_CHUNK;
    double s = 0.0;
    if ((t.numel & 3) == 0) {
        const int64_t n4 = t.numel >> 2;
        f32x4 g[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t i = (base >> 2) + k * SISR_BLOCK + threadIdx.x;
            g[k] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (i < n4) g[k] = reinterpret_cast<const f32x4*>(t.g)[i];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j) s += (double)g[k][j] * (double)g[k][j];
    } else {
        for (int k = 0; k < 16; ++k) {
            const int64_t i = base + k * SISR_BLOCK + threadIdx.x;
            if (i < t.numel) { const double g = (double)t.g[i]; s += g * g; }
        }
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double r = red[0];
#pragma unroll
        for (int w = 1; w < SISR_BLOCK / 64; ++w) r += red[w];
        part[blockIdx.x] = r;
    }
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
    __shared__ double red[SISR_BLOCK];
    const int tid = threadIdx.x;
    float norm_f = 0.f, coef = 1.f;
    int skip = 0;
    if (n_part > 0) {
        double s = 0.0;
        for (int64_t i = tid; i < n_part; i += SISR_BLOCK) s += part[i];
        red[tid] = s;
        __syncthreads();
        for (int o = SISR_BLOCK / 2; o > 0; o >>= 1) {
            if (tid < o) red[tid] += red[tid + o];
            __syncthreads();
        }
        const double norm = sqrt(red[0]);
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
    const int ti = adam_find_tensor(table, n, (int64_t)blockIdx.x);
    const SisrAdamDesc t = table[ti];
    const int64_t base = ((int64_t)blockIdx.x - t.block_start) * ADAM_CHUNK;
    adam_update_block<true>(t, base, ctrl[ADAM_CTRL_COEF], consts[2 * ti], omb1, beta2, omb2, eps, wd, consts[2 * ti + 1]);
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

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// 16-byte accesses need every element of both tensors on a 16-byte line: a parameter may be a view at an odd element offset
__device__ __forceinline__ bool ema_vec_ok(const SisrEmaDesc& t) {
    return (t.numel & 3) == 0 && ((reinterpret_cast<uintptr_t>(t.ema) | reinterpret_cast<uintptr_t>(t.src)) & 15) == 0;
}

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

// one workgroup per ADAM_CHUNK elements; all loads of a thread are issued before its first store
__global__ void __launch_bounds__(SISR_BLOCK) ema_update_kernel(const SisrEmaDesc* __restrict__ table, int n,
                                                                 const float* __restrict__ ctrl) {
    if (reinterpret_cast<const int*>(ctrl)[EMA_CTRL_ACTIVE] == 0) return;          // before any store
    const float omd = ctrl[EMA_CTRL_OMD];
    const SisrEmaDesc t = table[adam_find_tensor(table, n, (int64_t)blockIdx.x)];
    const int64_t base = ((int64_t)blockIdx.x - t.block_start) * ADAM_CHUNK;
    if (ema_vec_ok(t)) {
        const int64_t n4 = t.numel >> 2;
        const int64_t i0 = (base >> 2) + threadIdx.x;
        if (t.mode == 0) {
            f32x4 e[4], p[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t i = i0 + k * SISR_BLOCK;
                if (i < n4) { e[k] = reinterpret_cast<const f32x4*>(t.ema)[i]; p[k] = reinterpret_cast<const f32x4*>(t.src)[i]; }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t i = i0 + k * SISR_BLOCK;
                if (i < n4) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) e[k][j] = ema_value(e[k][j], p[k][j], omd);
                    reinterpret_cast<f32x4*>(t.ema)[i] = e[k];
                }
            }
        } else {
            u32x4 p[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t i = i0 + k * SISR_BLOCK;
                if (i < n4) p[k] = reinterpret_cast<const u32x4*>(t.src)[i];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t i = i0 + k * SISR_BLOCK;
                if (i < n4) reinterpret_cast<u32x4*>(t.ema)[i] = p[k];
            }
        }
    } else if (t.mode == 0) {
        for (int k = 0; k < 16; ++k) {
            const int64_t i = base + k * SISR_BLOCK + threadIdx.x;
            if (i < t.numel) t.ema[i] = ema_value(t.ema[i], t.src[i], omd);
        }
    } else {
        for (int k = 0; k < 16; ++k) {
            const int64_t i = base + k * SISR_BLOCK + threadIdx.x;
            if (i < t.numel) reinterpret_cast<unsigned*>(t.ema)[i] = reinterpret_cast<const unsigned*>(t.src)[i];
        }
    }
}

__global__ void __launch_bounds__(SISR_BLOCK) ema_swap_kernel(const SisrEmaDesc* __restrict__ table, int n) {
    const SisrEmaDesc t = table[adam_find_tensor(table, n, (int64_t)blockIdx.x)];
    const int64_t base = ((int64_t)blockIdx.x - t.block_start) * ADAM_CHUNK;
    if (ema_vec_ok(t)) {
        const int64_t n4 = t.numel >> 2;
        const int64_t i0 = (base >> 2) + threadIdx.x;
        u32x4 e[4], p[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t i = i0 + k * SISR_BLOCK;
            if (i < n4) { e[k] = reinterpret_cast<const u32x4*>(t.ema)[i]; p[k] = reinterpret_cast<const u32x4*>(t.src)[i]; }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t i = i0 + k * SISR_BLOCK;
            if (i < n4) { reinterpret_cast<u32x4*>(t.ema)[i] = p[k]; reinterpret_cast<u32x4*>(t.src)[i] = e[k]; }
        }
    } else {
        unsigned* ema = reinterpret_cast<unsigned*>(t.ema);
        unsigned* src = reinterpret_cast<unsigned*>(t.src);
        for (int k = 0; k < 16; ++k) {
            const int64_t i = base + k * SISR_BLOCK + threadIdx.x;
            if (i < t.numel) { const unsigned e = ema[i], p = src[i]; ema[i] = p; src[i] = e; }
        }
    }
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
