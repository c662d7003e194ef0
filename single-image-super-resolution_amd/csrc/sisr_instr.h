// sisr_instr.h -- developer instrumentation of the kernels; everything here compiles to nothing in the production build.
//   make trace (-DSISR_CONV_TRACE; tools/trace_*.py): phase timelines -- chosen threads stamp a clock into their workgroup's row
//     of a device buffer, which an extern "C" reader copies out.
//   make acct (-DSISR_BARRIER_ACCT; tools/barrier_acct.py): barrier-wait accounting -- every tile-loop barrier is bracketed by
//     two s_memtime reads whose difference is summed in SGPRs (no stores, no LDS drain inside the loop); one lane per role
//     stores {loop cycles, cycles spent waiting at barriers} at the end.
#pragma once
#include <hip/hip_runtime.h>

// buffer NAME_buf of n unsigned 64-bit words and its reader NAME_read(dst, n_u64)
#define SISR_INSTR_BUFFER(name, n)                                                                                       \
    __device__ unsigned long long name##_buf[n];                                                                         \
    extern "C" int name##_read(void* dst, int n_u64) {                                                                   \
        return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(name##_buf), (size_t)n_u64 * 8, 0, hipMemcpyDeviceToHost);       \
    }

#ifdef SISR_CONV_TRACE
// timeline buffer NAME_buf [wgs][slots]
#define SISR_TRACE_BUFFER(name, wgs, slots)                      \
    static constexpr int name##_wgs = wgs, name##_slots = slots; \
    SISR_INSTR_BUFFER(name, wgs * slots)
// the threads for which `who` holds store `clk` (wall_clock64(): 100 MHz; clock64(): s_memtime) into slot `slot` of row `wg`;
// slots from `end` on belong to someone else (another role's half of the row, the next row)
#define SISR_TRACE_STAMP(name, who, wg, slot, end, clk)                                                             \
    do {                                                                                                            \
        if ((who) && (wg) < name##_wgs && (slot) < (end)) name##_buf[(wg) * name##_slots + (slot)] = clk;            \
    } while (0)
// the same with the row computed once, ahead of the tests: for rows that take arithmetic (2-D grids)
#define SISR_TRACE_STAMP_ROW(name, who, wg, slot, end, clk)    \
    do {                                                       \
        const auto wg_ = (wg);                                 \
        SISR_TRACE_STAMP(name, who, wg_, slot, end, clk);      \
    } while (0)
#else
#define SISR_TRACE_BUFFER(name, wgs, slots)
#define SISR_TRACE_STAMP(name, who, wg, slot, end, clk)
#define SISR_TRACE_STAMP_ROW(name, who, wg, slot, end, clk)
#endif

#ifdef SISR_BARRIER_ACCT
// accounting buffer NAME_buf [512 workgroups][per_wg]
#define SISR_ACCT_BUFFER(name, per_wg)         \
    static constexpr int name##_per_wg = per_wg; \
    SISR_INSTR_BUFFER(name, 512 * per_wg)
// (SISR_ACCT_SYNC and SISR_ACCT_STORE use the two locals of the SISR_ACCT_DECL in scope)
#define SISR_ACCT_DECL unsigned long long ba_wait = 0, ba_t0 = clock64()
#define SISR_ACCT_SYNC() do { const unsigned long long b0_ = clock64(); __syncthreads(); ba_wait += clock64() - b0_; } while (0)
// lane 0 of the calling wave: cycles since SISR_ACCT_DECL into `slot`, cycles waited at SISR_ACCT_SYNC into `slot` + 1
#define SISR_ACCT_STORE(name, slot)                                            \
    do {                                                                       \
        if ((threadIdx.x & 63) == 0 && blockIdx.x < 512) {                     \
            name##_buf[blockIdx.x * name##_per_wg + (slot)] = clock64() - ba_t0; \
            name##_buf[blockIdx.x * name##_per_wg + (slot) + 1] = ba_wait;     \
        }                                                                      \
    } while (0)
// thread 0: the shader clock into `slot`
#define SISR_ACCT_MARK(name, slot) do { if (threadIdx.x == 0 && blockIdx.x < 512) name##_buf[blockIdx.x * name##_per_wg + (slot)] = clock64(); } while (0)
#else
#define SISR_ACCT_BUFFER(name, per_wg)
#define SISR_ACCT_DECL
#define SISR_ACCT_SYNC() __syncthreads()
#define SISR_ACCT_STORE(name, slot)
#define SISR_ACCT_MARK(name, slot)
#endif
