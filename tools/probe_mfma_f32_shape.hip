// probe_mfma_f32_shape.hip -- stand-alone probe (tools/probe_mfma_f32_shape.py): does the clock an exact-fp32 MFMA loop holds depend on
// the instruction's shape?  One workgroup per CU, four MFMA waves, random operands re-read from LDS with ds_read_b128 (two 16-byte
// reads per four MFMA-equivalents, the trunk kernels' ratio), the same 32 x 32 output per wave:
//   mode 0: one accumulation chain of v_mfma_f32_32x32x2_f32 (what conv_trunk_f32.hip / wgrad_trunk_f32.hip issue);
//   mode 1: four interleaved chains of v_mfma_f32_16x16x4_f32, one per 16 x 16 block of that output.
// One MFMA-equivalent = 2,048 multiply-adds = one 32x32x2 = two 16x16x4.  Lane 0 of every workgroup stamps the 100 MHz wall clock
// and the shader clock (s_memtime) around the loop: in-kernel clock = delta(s_memtime) / delta(wall) x 100 MHz.
#include <hip/hip_runtime.h>

typedef float pf_f32x4 __attribute__((ext_vector_type(4)));
typedef float pf_f32x16 __attribute__((ext_vector_type(16)));

#define PF_THREADS 256
#define PF_LDS_FLOATS 8192                 // 32 KB of operands
#define PF_UNROLL 8                        // operand pairs per loop iteration: 32 MFMA-equivalents

template <int MODE>
__global__ void __launch_bounds__(PF_THREADS) probe_mfma_kernel(const float* __restrict__ rnd, float* __restrict__ out,
                                                               unsigned long long* __restrict__ stamps, int iters) {
    __shared__ __attribute__((aligned(16))) float lds[PF_LDS_FLOATS];
    const int tid = threadIdx.x, lane = tid & 63;
    for (int i = tid; i < PF_LDS_FLOATS; i += PF_THREADS) lds[i] = rnd[i];
    __syncthreads();
    // a lane's operands: 16 bytes of A and 16 of B per pair, 144-byte lane stride (conflict-free, as the trunk kernels' rows)
    const float* pa = lds + lane * 36;
    const float* pb = lds + 4096 + lane * 36;
    pf_f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    unsigned long long w0 = 0, c0 = 0;
    if (tid == 0) { w0 = wall_clock64(); c0 = clock64(); }
    for (int it = 0; it < iters; ++it) {
        pf_f32x4 a[PF_UNROLL], b[PF_UNROLL];
#pragma unroll
        for (int u = 0; u < PF_UNROLL; ++u) {
            a[u] = *reinterpret_cast<const pf_f32x4*>(pa + 4 * ((u + it) & 7));
            b[u] = *reinterpret_cast<const pf_f32x4*>(pb + 4 * ((u + 3 * it) & 7));
        }
#pragma unroll
        for (int u = 0; u < PF_UNROLL; ++u) {
            if (MODE == 0) {
#pragma unroll
                for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u][s], b[u][s], acc, 0, 0, 0);
            } else {
                // chain 2 i + j = block (i, j) of the output: registers 4 (2 i + j) .. + 3 of acc
#pragma unroll
                for (int r = 0; r < 2; ++r)
#pragma unroll
                    for (int ij = 0; ij < 4; ++ij) {
                        pf_f32x4 c = {acc[4 * ij], acc[4 * ij + 1], acc[4 * ij + 2], acc[4 * ij + 3]};
                        c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][2 * r + (ij >> 1)], b[u][2 * r + (ij & 1)], c, 0, 0, 0);
                        acc[4 * ij] = c[0]; acc[4 * ij + 1] = c[1]; acc[4 * ij + 2] = c[2]; acc[4 * ij + 3] = c[3];
                    }
            }
        }
    }
    if (tid == 0) {
        const unsigned long long w1 = wall_clock64(), c1 = clock64();
        stamps[2 * blockIdx.x] = w1 - w0;
        stamps[2 * blockIdx.x + 1] = c1 - c0;
    }
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) s += acc[i];
    out[(size_t)blockIdx.x * PF_THREADS + tid] = s;            // (keeps the chains alive)
}

// rnd: PF_LDS_FLOATS floats; out: grid * 256 floats; stamps: grid * 2 words {wall ticks, shader-clock ticks}
extern "C" int probe_mfma_f32_shape(int mode, int grid, int iters, const float* rnd, float* out, unsigned long long* stamps, hipStream_t st) {
    if (grid < 1 || iters < 1 || !rnd || !out || !stamps) return -1;
    if (mode == 0)
        probe_mfma_kernel<0><<<dim3(grid), dim3(PF_THREADS), 0, st>>>(rnd, out, stamps, iters);
    else
        probe_mfma_kernel<1><<<dim3(grid), dim3(PF_THREADS), 0, st>>>(rnd, out, stamps, iters);
    return (int)hipGetLastError();
}

extern "C" int probe_mfma_equivalents_per_iter() { return PF_UNROLL * 4; }
