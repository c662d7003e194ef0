// sisr_cubic.h -- the cubic-convolution taps of F.interpolate(mode='bicubic', align_corners=True) as ATen's UpSampleBicubic2d
// computes them (A = -0.75, src = scale * dst, 4 taps at floor(src) - 1 .. + 2 clamped to the image), shared by resample.hip
// (utils.lr_from_hr) and degrade.hip (blur + resample + noise): one text, so the two operators resample identically.
#pragma once

#define CUBIC_A (-0.75f)
__device__ __forceinline__ float cc1(float x) { return ((CUBIC_A + 2.f) * x - (CUBIC_A + 3.f)) * x * x + 1.f; }
__device__ __forceinline__ float cc2(float x) { return ((CUBIC_A * x - 5.f * CUBIC_A) * x + 8.f * CUBIC_A) * x - 4.f * CUBIC_A; }

__device__ __forceinline__ void cubic_setup(int dst, float scale, int n_in, int idx[4], float w[4]) {
    const float src = scale * (float)dst;
    const float fl = floorf(src);
    const int i0 = (int)fl;
    const float t = src - fl;
    w[0] = cc2(t + 1.f); w[1] = cc1(t); w[2] = cc1(1.f - t); w[3] = cc2(2.f - t);
#pragma unroll
    for (int k = 0; k < 4; ++k) idx[k] = min(max(i0 - 1 + k, 0), n_in - 1);
}

// weight with which output index `o` reads input index `i` along one axis (taps that the border clamp folds onto
// the same input index add up)
__device__ __forceinline__ float cubic_weight_of(int o, float scale, int n_in, int i) {
    int idx[4];
    float w[4];
    cubic_setup(o, scale, n_in, idx, w);
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) s += idx[k] == i ? w[k] : 0.f;
    return s;
}

// output indices whose 4 taps can reach input index i: floor(scale * o) in [i - 2, i + 1] (one index of margin
// on each side; cubic_weight_of() returns 0 for the ones that do not)
__device__ __forceinline__ void cubic_reach(int i, float scale, int n_out, int& lo, int& hi) {
    if (scale > 0.f) {
        lo = max(0, (int)floorf((float)(i - 2) / scale) - 1);
        hi = min(n_out - 1, (int)ceilf((float)(i + 2) / scale) + 1);
    } else {
        lo = 0; hi = n_out - 1;
    }
}

static inline float ac_scale(int n_in, int n_out) { return n_out > 1 ? (float)(n_in - 1) / (float)(n_out - 1) : 0.f; }
