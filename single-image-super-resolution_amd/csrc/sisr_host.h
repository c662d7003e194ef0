// sisr_host.h -- host-side helpers shared by the .hip files: per-device state, kernel launch, environment switches, and the
// host entry points that one file defines and another calls (the public ABI is ../../include/sisr_hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdlib>
#include "../../include/sisr_hip.h"

#define SISR_CHECK_LAUNCH()                          \
    do {                                             \
        hipError_t e__ = hipGetLastError();          \
        if (e__ != hipSuccess) return (int)e__;      \
    } while (0)

static inline hipStream_t sisr_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// A/B switch NAME=0 (keeps the generic kernel, the fp32 slabs, ...).  Read at every call: tests flip switches inside one process.
static inline bool sisr_switch_off(const char* name) {
    const char* e = getenv(name);
    return e && e[0] == '0';
}

// ---- per-device state -----------------------------------------------------------------------------------------------
// One process normally drives one GPU (one rank per device), but nothing below assumes it: the CU count and the
// dynamic-LDS caps are kept per device id, so a host that switches devices (the reference's nn.DataParallel,
// config.py:114-118) gets correct grids and attributes on each.
#define SISR_MAX_DEVICES 64
int sisr_device_index();                   // misc.hip: current device id, clamped to [0, SISR_MAX_DEVICES)
// misc.hip: workgroup slots a persistent kernel may fill = CUs of the CURRENT device.  SISR_PERSIST_MAX_WG=<n> caps it
// (test knob: a small cap makes a small input walk many tiles per workgroup, the schedule of the full-size launches)
int sisr_cu_slots();
// equal shares: workgroups of a persistent kernel that walks `total` tiles on `slots` workgroup slots.  Every workgroup walks
// rounds = ceil(total / slots) tiles, so ceil(total / rounds) of them cover the tiles with no slot idle for a whole round.
static inline int sisr_equal_shares(int total, int slots, int* rounds_out = nullptr) {
    if (slots < 1) slots = 1;
    const int rounds = (total + slots - 1) / slots;
    if (rounds_out) *rounds_out = rounds;
    return (total + rounds - 1) / rounds;
}
struct SisrLdsCap { int v[SISR_MAX_DEVICES]; };
// raise hipFuncAttributeMaxDynamicSharedMemorySize of `fn` on the current device when `bytes` exceeds what was set
// (`base`: the cap a kernel starts with -- 64 KB without the attribute, 0 forces the first call to set it)
#define SISR_LDS_BASE_DEFAULT (64 * 1024)
static inline int sisr_raise_lds_cap(SisrLdsCap& cap, const void* fn, int bytes, int base) {
    int& cur = cap.v[sisr_device_index()];
    if (cur < base) cur = base;
    if (bytes <= cur) return 0;
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) return (int)e;
    cur = bytes;
    return 0;
}
// launch kernel K with `lds` bytes of dynamic LDS: raises K's cap first (one SisrLdsCap per kernel, this function's static),
// returns the launch error or 0
template <auto K, typename... Args>
static int sisr_launch(dim3 grid, dim3 block, int lds, int lds_base, hipStream_t st, const Args&... args) {
    static SisrLdsCap cap;
    if (int e = sisr_raise_lds_cap(cap, reinterpret_cast<const void*>(K), lds, lds_base)) return e;
    hipLaunchKernelGGL(K, grid, block, lds, st, args...);
    SISR_CHECK_LAUNCH();
    return 0;
}

// ---- host entry points called across files: the dispatchers hand a routed descriptor to the specialised kernel's file, and ask it
// for the grid its launch will have ------------------------------------------------------------------------------------------------
int sisr_conv2d_trunk_launch(const SisrConvDesc* d, hipStream_t st);          // conv_trunk.hip
int sisr_conv2d_trunk_grid(const SisrConvDesc* d);                            // conv_trunk.hip: workgroups
int sisr_conv2d_trunk_f32_launch(const SisrConvDesc* d, hipStream_t st);      // conv_trunk_f32.hip
int sisr_conv2d_trunk_f32_streams(const SisrConvDesc* d);                     // conv_trunk_f32.hip: pixel-tile streams
int sisr_conv2d_thin_launch(const SisrConvDesc* d, hipStream_t st);           // conv_thin.hip
int sisr_conv2d_toimage_launch(const SisrConvDesc* d, hipStream_t st);        // conv_toimage.hip
int sisr_conv2d_deep_launch(const SisrConvDesc* d, hipStream_t st);           // conv_deep.hip
int sisr_conv2d_deep_parts(const SisrConvDesc* d);                            // conv_deep.hip
int sisr_wgrad_trunk_launch(const SisrWgradDesc* d, hipStream_t st);          // wgrad_trunk.hip
int sisr_wgrad_trunk_slabs(const SisrWgradDesc* d);                           // wgrad_trunk.hip
int sisr_wgrad_trunk_f32_launch(const SisrWgradDesc* d, hipStream_t st);      // wgrad_trunk_f32.hip
int sisr_wgrad_trunk_f32_slabs(const SisrWgradDesc* d);                       // wgrad_trunk_f32.hip
int sisr_wgrad_thin_launch(const SisrWgradDesc* d, hipStream_t st);           // wgrad_thin.hip
int sisr_wgrad_thin_slabs(const SisrWgradDesc* d);                            // wgrad_thin.hip
int sisr_wgrad_toimage_launch(const SisrWgradDesc* d, hipStream_t st);        // wgrad_toimage.hip
int sisr_wgrad_toimage_f32_launch(const SisrWgradDesc* d, hipStream_t st);    // wgrad_toimage.hip
int sisr_wgrad_toimage_slabs(const SisrWgradDesc* d);                         // wgrad_toimage.hip
int sisr_wgrad_deep_launch(const SisrWgradDesc* d, hipStream_t st);           // wgrad_deep.hip
