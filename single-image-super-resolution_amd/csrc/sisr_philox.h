// sisr_philox.h -- what the device-side samplers (patchsrc.hip, degrade.hip, jpeg.hip, resize.hip) share: the generator, the one
// counter layout (draw_words), the uniforms, the categorical pick, the list of word-3 tags (DrawTag) and the step protocol of the
// advancing draw kernels.  One text for host and device: every draw has a host restatement that needs no GPU.  Python mirror: draws.py.
#pragma once
#include <math.h>
#include <stdint.h>

// ---- Philox4x32-10 -------------------------------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ uint32_t patch_mulhi32(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) >> 32); }

__host__ __device__ __forceinline__ void philox4x32_10(const uint32_t ctr[4], uint32_t k0, uint32_t k1, uint32_t out[4]) {
    uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3];
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = patch_mulhi32(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = patch_mulhi32(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// ---- whose counter: word 3 -------------------------------------------------------------------------------------------------------
// A patch-source sample carries its rank (< 2^31) in word 3; every other stream carries tag | rank with rank < DRAW_RANK_LIMIT, or
// one of the two permutation forms.  A new sampler takes the next 0xFExx0000 here and nowhere else.
#define PATCH_PERM_ROUNDS 24
enum DrawTag : uint32_t {
    DRAW_TAG_PARAMS = 0xFE010000u,         // degrade.hip: a sample's sigma1, sigma2, theta, sigma_n
    DRAW_TAG_NOISE = 0xFE020000u,          // degrade.hip: four colour noise values (word 2: element / 4)
    DRAW_TAG_QUALITY = 0xFE030000u,        // jpeg.hip: a sample's quality
    DRAW_TAG_MIX_A = 0xFE040000u,          // degrade.hip, mixed draw: blur on, k_eff, sinc, family
    DRAW_TAG_MIX_B = 0xFE050000u,          //   sigma1, sigma2, theta, beta
    DRAW_TAG_MIX_C = 0xFE060000u,          //   omega, noise mode, grey, amplitude
    DRAW_TAG_MIX_FINAL = 0xFE070000u,      //   the final filter: sinc, k_eff, omega
    DRAW_TAG_NOISE_GREY = 0xFE080000u,     // degrade.hip: four grey noise values (word 2: pixel / 4)
    DRAW_TAG_MODE = 0xFE090000u,           // resize.hip: a sample's resampler
    DRAW_TAG_PERM_BIT = 0xFFFFFFFEu,       // patchsrc.hip: the swap bit of round r is tagged DRAW_TAG_PERM_BIT - r (word 2: the pair's larger member)
    DRAW_TAG_PERM_KEY = 0xFFFFFFFFu,       // patchsrc.hip: the round keys of an epoch (word 2: the round); the epoch stands in for t
};
constexpr int DRAW_RANK_LIMIT = 1 << 16;

// every tag that is or-ed with a rank: low 16 bits zero (tag | rank keeps both), at or above 2^31 (above every patch-source rank),
// with any rank below the permutation tags, and ascending from `below` on, hence pairwise distinct
constexpr bool draw_tag_ok(uint32_t below, uint32_t tag) {
    return !(tag & (DRAW_RANK_LIMIT - 1)) && tag >= 0x80000000u && tag > below &&
           tag + (DRAW_RANK_LIMIT - 1) < DRAW_TAG_PERM_BIT - (PATCH_PERM_ROUNDS - 1);
}
static_assert(draw_tag_ok(0, DRAW_TAG_PARAMS) && draw_tag_ok(DRAW_TAG_PARAMS, DRAW_TAG_NOISE) && draw_tag_ok(DRAW_TAG_NOISE, DRAW_TAG_QUALITY) &&
              draw_tag_ok(DRAW_TAG_QUALITY, DRAW_TAG_MIX_A) && draw_tag_ok(DRAW_TAG_MIX_A, DRAW_TAG_MIX_B) && draw_tag_ok(DRAW_TAG_MIX_B, DRAW_TAG_MIX_C) &&
              draw_tag_ok(DRAW_TAG_MIX_C, DRAW_TAG_MIX_FINAL) && draw_tag_ok(DRAW_TAG_MIX_FINAL, DRAW_TAG_NOISE_GREY) &&
              draw_tag_ok(DRAW_TAG_NOISE_GREY, DRAW_TAG_MODE), "a 0xFE.. tag breaks the rules of the tag list");

// ---- one draw ----------------------------------------------------------------------------------------------------------------------
// the four words of counter {t low, t high, word2, word3} under key {seed low, seed high}
__host__ __device__ __forceinline__ void draw_words(uint64_t seed, int64_t t, uint32_t word2, uint32_t word3, uint32_t out[4]) {
    const uint32_t ctr[4] = {(uint32_t)((uint64_t)t & 0xFFFFFFFFu), (uint32_t)((uint64_t)t >> 32), word2, word3};
    philox4x32_10(ctr, (uint32_t)(seed & 0xFFFFFFFFu), (uint32_t)(seed >> 32), out);
}

// u = ((r >> 8) + 0.5) 2^-24, in (0, 1]: fp32 rounds the 25-bit numerator to even above 1/2, so the last value reads as 1
__host__ __device__ __forceinline__ float draw_uniform(uint32_t r) { return ((float)(r >> 8) + 0.5f) * (1.0f / 16777216.0f); }

// ln u for the same word.  Below 1/2 the numerator is exact and logf takes it; above, 1 - u = (2^24 - (r >> 8) - 0.5) 2^-24 is the
// exact quantity and log1pf takes that: near u = 1, where a Box-Muller radius is sqrt(2 (1 - u)), the rounded u would carry an
// error as large as the radius itself
__host__ __device__ __forceinline__ float draw_log_uniform(uint32_t r) {
    const uint32_t m = r >> 8;
    if (m < (1u << 23)) return logf(((float)m + 0.5f) * (1.0f / 16777216.0f));
    return log1pf(-(((float)((1u << 24) - m) - 0.5f) * (1.0f / 16777216.0f)));
}

// the first i with p_i > 0 and u <= p_0 + .. + p_i (fp32, added in index order); u above the rounded sum: the last i with p_i > 0
__host__ __device__ __forceinline__ int draw_pick(const float* p, int n, float u) {
    float c = 0.f;
    int m = 0;
    for (int i = 0; i < n; ++i) {
        if (p[i] > 0.f) m = i;
        c += p[i];
        if (p[i] > 0.f && u <= c) break;
    }
    return m;
}

// ---- the step protocol of an advancing draw kernel (one workgroup) -----------------------------------------------------------------
// Every thread reads the count; what the kernel leaves in LDS goes between the two calls; draw_step_advance is the kernel's one barrier,
// behind which one thread stores count + 1 and, where asked, the step just drawn: a captured draw advances on every replay.
__device__ __forceinline__ int64_t draw_step_read(const int64_t* step) { return *step; }
__device__ __forceinline__ void draw_step_advance(int64_t* step, int64_t t, int64_t* drawn_step) {
    __syncthreads();
    if (threadIdx.x == 0) {
        *step = t + 1;
        if (drawn_step != nullptr) drawn_step[0] = t;
    }
}
