// sisr_philox.h -- the counter-based random numbers of the device-side samplers (patchsrc.hip, degrade.hip, jpeg.hip, resize.hip): one text for host and
// device, so every draw has a host restatement that needs no GPU.  Word 3 of a counter says whose it is: a patch-source sample
// carries its rank (< 2^31), the epoch permutation tags >= 0xFFFFFFE7, the degradation 0xFE01xxxx / 0xFE02xxxx (degrade.hip), the
// JPEG quality 0xFE03xxxx (jpeg.hip), the mixed kernel draw 0xFE04xxxx .. 0xFE07xxxx (family and size, shape, cutoff and noise row,
// final filter), the grey noise 0xFE08xxxx (degrade.hip) and the resize mode 0xFE09xxxx (resize.hip).  The next free tag is 0xFE0Axxxx.
#pragma once
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
