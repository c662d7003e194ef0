// sisr_ssim_bwd.h -- the backward SSIM tile scheme, once, for its two callers: the image loss (image_loss.hip) and every level of
// MS-SSIM (ms_ssim.hip).  Gather form, nothing saved by a forward but the inputs.  Per window position q with moments mu_a, mu_b,
// E_aa, E_bb, E_ab:  A1 = 2 mu_a mu_b + C1, A2 = 2 (E_ab - mu_a mu_b) + C2, B1 = mu_a^2 + mu_b^2 + C1,
// B2 = (E_aa - mu_a^2) + (E_bb - mu_b^2) + C2, and for the map S = l cs = A1 A2 / (B1 B2) (SSIM_MAP_LCS)
//   D_e = dS/dE_ab = 2 A1 / (B1 B2),   D_q = dS/dE_aa = dS/dE_bb = -S / B2,
//   D_mua = 2 mu_b (A2 - A1) / (B1 B2) + 2 mu_a S (1 / B2 - 1 / B1),   D_mub: mu_a and mu_b exchanged;
// for the map cs = A2 / B2 (SSIM_MAP_CS, the levels of MS-SSIM but the last)
//   D_e = 2 / B2,   D_q = -cs / B2,   D_mua = 2 (cs mu_a - mu_b) / B2,   D_mub: mu_a and mu_b exchanged.
// With T the transposed window (the same symmetric taps over a map that is zero outside the valid positions):
//   d(sum_q S)/da(p) = T(D_mua)(p) + 2 a(p) T(D_q)(p) + b(p) T(D_e)(p),   db: a and b exchanged.
// A workgroup owns an SSIM_TH x SSIM_TW tile of pixels of one (image, plane) of the WHOLE image (so a cropped border is written
// too: exact zeros).  ssim_bwd_filter_maps stages the SSIM_BH x SSIM_BW pixels around the tile, recomputes the moments at the
// SSIM_SH x SSIM_SW positions whose windows touch the tile, leaves the derivative maps in LDS and filters them along the rows;
// ssim_bwd_pixels walks the tile's pixels, hands each one inside the view to the caller and stores what comes back (under luma
// all three channel gradients); the caller's lambda takes the UNSCALED window gradient of its pixel from ssim_bwd_window_grad,
// multiplies by its own factor and adds its own term.
// LDS (SsimBwdLds, declared by the kernel): 2 x 36 x 52 staged pixels (15.0 KB) + 5 x 36 x 42 row-filtered moments (30.2 KB, reused
// for the row-filtered derivative maps) + 4 x 26 x 42 derivative maps (17.5 KB) = 62,688 B per workgroup.
//
// Rounding, the one rule for the SSIM files: sisr_ssim.h (the forward) is compiled under the compiler's default contraction, the
// way metrics.hip compiles it, so it is included FIRST; from the pragma below to the end of the including file every product and
// sum is rounded as written (fused multiply-adds are spelled fmaf).  The instantiations of a backward kernel then compute a
// gradient with the same operations, so da is the same bits whether or not db is asked for, and both callers get the same bits
// from this text.
#pragma once
#include "sisr_ssim.h"

#include <type_traits>

#pragma clang fp contract(off)

#define SSIM_BH (SSIM_TH + 2 * SSIM_APRON)    // backward: staged pixels
#define SSIM_BW (SSIM_TW + 2 * SSIM_APRON)
#define SSIM_MAP_LCS 0                        // the SSIM map l cs
#define SSIM_MAP_CS 1                         // cs alone

struct SsimBwdLds {
    float sa[SSIM_BH * SSIM_BW], sb[SSIM_BH * SSIM_BW];
    float hm[5 * SSIM_BH * SSIM_SW];          // row-filtered moments [5][SSIM_BH][SSIM_SW], then maps [NM][SSIM_SH][SSIM_TW]
    float dm[4][SSIM_SH * SSIM_SW];           // derivative maps: D_q, D_e, D_mua and / or D_mub
};
static_assert(4 * SSIM_SH * SSIM_TW <= 5 * SSIM_BH * SSIM_SW, "the row-filtered derivative maps reuse the moments' LDS");

// number of derivative maps and the indices of D_mua / D_mub among them
template <bool WA, bool WB>
struct SsimBwdMaps {
    static constexpr int NM = 2 + (WA ? 1 : 0) + (WB ? 1 : 0), MA = 2, MB = WA ? 3 : 2;
};

// one pixel of the view; off: the element of the first plane
__device__ __forceinline__ float ssim_view_load(const float* __restrict__ p, int64_t off, int64_t plane_elems, int luma) {
    return luma ? fmaf(0.114f, p[off + 2 * plane_elems], fmaf(0.587f, p[off + plane_elems], 0.299f * p[off])) : p[off];
}

// workgroup = (image n, plane, pixel-tile row, pixel-tile column) of the WHOLE image, flat in that order
struct SsimBwdTile {
    int n, plane;
    int cy0, cx0;                             // tile origin in the view's coordinates (< 0 in the border)
    int64_t plane_elems, base;
};

__device__ __forceinline__ SsimBwdTile ssim_bwd_tile(const SsimGeom& g) {
    const SsimTile t = ssim_tile(g, g.btiles_y, g.btiles_x);
    return {t.n, t.plane, t.ty * SSIM_TH - g.crop, t.tx * SSIM_TW - g.crop, t.plane_elems, t.base};
}

// the pixels under every window that touches the tile; outside the view: zeros
__device__ __forceinline__ void ssim_bwd_stage(const float* __restrict__ a, const float* __restrict__ b, const SsimGeom& g,
                                               const SsimBwdTile& t, SsimBwdLds& s) {
    for (int i = threadIdx.x; i < SSIM_BH * SSIM_BW; i += SISR_BLOCK) {
        const int ly = i / SSIM_BW, lx = i - ly * SSIM_BW;
        const int y = t.cy0 - SSIM_APRON + ly, x = t.cx0 - SSIM_APRON + lx;
        float va = 0.f, vb = 0.f;
        if (y >= 0 && y < g.Hc && x >= 0 && x < g.Wc) {
            const int64_t off = t.base + (int64_t)(y + g.crop) * g.W + (x + g.crop);
            va = ssim_view_load(a, off, t.plane_elems, g.luma);
            vb = ssim_view_load(b, off, t.plane_elems, g.luma);
        }
        s.sa[i] = va;
        s.sb[i] = vb;
    }
}

// horizontal pass: the five moments of every staged row at the SSIM_SW position columns (lanes on consecutive columns)
__device__ __forceinline__ void ssim_bwd_row_pass(const SsimWindow& win, SsimBwdLds& s) {
    for (int i = threadIdx.x; i < SSIM_BH * SSIM_SW; i += SISR_BLOCK) {
        const int ly = i / SSIM_SW, ox = i - ly * SSIM_SW;
        const float* pa = s.sa + ly * SSIM_BW + ox;
        const float* pb = s.sb + ly * SSIM_BW + ox;
        float ma = 0.f, mb = 0.f, maa = 0.f, mbb = 0.f, mab = 0.f;
#pragma unroll
        for (int k = 0; k < SSIM_WIN; ++k) {
            const float w = win.w[k], u = pa[k], v = pb[k];
            const float wu = w * u, wv = w * v;
            ma += wu; mb += wv;
            maa = fmaf(wu, u, maa); mbb = fmaf(wv, v, mbb); mab = fmaf(wu, v, mab);
        }
        s.hm[i] = ma; s.hm[SSIM_BH * SSIM_SW + i] = mb; s.hm[2 * (SSIM_BH * SSIM_SW) + i] = maa;
        s.hm[3 * (SSIM_BH * SSIM_SW) + i] = mbb; s.hm[4 * (SSIM_BH * SSIM_SW) + i] = mab;
    }
}

// vertical pass + derivative maps at the SSIM_SH x SSIM_SW positions (position (qy, qx) = view position
// (cy0 - 10 + qy, cx0 - 10 + qx)); i + k SSIM_SW: lanes on consecutive addresses
template <bool WA, bool WB, int MAP>
__device__ __forceinline__ void ssim_bwd_col_pass_maps(const SsimGeom& g, const SsimWindow& win, float c1, float c2,
                                                       const SsimBwdTile& t, SsimBwdLds& s) {
    constexpr int MA = SsimBwdMaps<WA, WB>::MA, MB = SsimBwdMaps<WA, WB>::MB;
    for (int i = threadIdx.x; i < SSIM_SH * SSIM_SW; i += SISR_BLOCK) {
        const int qy = i / SSIM_SW, qx = i - qy * SSIM_SW;
        float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < SSIM_WIN; ++k) {
            const float w = win.w[k];
#pragma unroll
            for (int q = 0; q < 5; ++q) m[q] = fmaf(w, s.hm[q * (SSIM_BH * SSIM_SW) + i + k * SSIM_SW], m[q]);
        }
        const int py = t.cy0 - SSIM_APRON + qy, px = t.cx0 - SSIM_APRON + qx;
        const bool valid = py >= 0 && py < g.Hv && px >= 0 && px < g.Wv;
        const float mu_aa = m[0] * m[0], mu_bb = m[1] * m[1], mu_ab = m[0] * m[1];
        const float a2 = fmaf(2.f, m[4] - mu_ab, c2);
        const float rb2 = 1.f / ((m[2] - mu_aa) + (m[3] - mu_bb) + c2);
        if constexpr (MAP == SSIM_MAP_LCS) {
            const float a1 = fmaf(2.f, mu_ab, c1);
            const float rb1 = 1.f / (mu_aa + mu_bb + c1);
            const float r12 = rb1 * rb2;
            const float ssim = a1 * a2 * r12;
            const float cross = 2.f * (a2 - a1) * r12, self = 2.f * ssim * (rb2 - rb1);
            s.dm[0][i] = valid ? -ssim * rb2 : 0.f;
            s.dm[1][i] = valid ? 2.f * a1 * r12 : 0.f;
            if (WA) s.dm[MA][i] = valid ? fmaf(m[1], cross, m[0] * self) : 0.f;
            if (WB) s.dm[MB][i] = valid ? fmaf(m[0], cross, m[1] * self) : 0.f;
        } else {
            const float cs = a2 * rb2;
            s.dm[0][i] = valid ? -cs * rb2 : 0.f;
            s.dm[1][i] = valid ? 2.f * rb2 : 0.f;
            if (WA) s.dm[MA][i] = valid ? 2.f * fmaf(cs, m[0], -m[1]) * rb2 : 0.f;
            if (WB) s.dm[MB][i] = valid ? 2.f * fmaf(cs, m[1], -m[0]) * rb2 : 0.f;
        }
    }
}

// transposed window, horizontal: pixel column px of the tile gathers positions px .. px + 10 (symmetric taps)
template <int NM>
__device__ __forceinline__ void ssim_bwd_row_window(const SsimWindow& win, SsimBwdLds& s) {
    for (int i = threadIdx.x; i < SSIM_SH * SSIM_TW; i += SISR_BLOCK) {
        const int qy = i / SSIM_TW, px = i - qy * SSIM_TW;
        float h[NM];
#pragma unroll
        for (int q = 0; q < NM; ++q) h[q] = 0.f;
#pragma unroll
        for (int k = 0; k < SSIM_WIN; ++k) {
            const float w = win.w[k];
#pragma unroll
            for (int q = 0; q < NM; ++q) h[q] = fmaf(w, s.dm[q][qy * SSIM_SW + px + k], h[q]);
        }
#pragma unroll
        for (int q = 0; q < NM; ++q) s.hm[q * (SSIM_SH * SSIM_TW) + i] = h[q];
    }
}

// the four phases in front of the per-pixel one, with their barriers; the last barrier is behind the last phase
template <bool WA, bool WB, int MAP>
__device__ __forceinline__ void ssim_bwd_filter_maps(const float* __restrict__ a, const float* __restrict__ b, const SsimGeom& g,
                                                     const SsimWindow& win, float c1, float c2, const SsimBwdTile& t, SsimBwdLds& s) {
    ssim_bwd_stage(a, b, g, t, s);
    __syncthreads();
    ssim_bwd_row_pass(win, s);
    __syncthreads();
    ssim_bwd_col_pass_maps<WA, WB, MAP>(g, win, c1, c2, t, s);
    __syncthreads();
    ssim_bwd_row_window<SsimBwdMaps<WA, WB>::NM>(win, s);
    __syncthreads();
}

// transposed window, vertical, at pixel (py, px) of the tile -> the staged pixel (va, vb) and the UNSCALED window gradient
// (wa, wb) = d(sum_q map)/d(a, b)(p); the one not asked for is left alone
template <bool WA, bool WB>
__device__ __forceinline__ void ssim_bwd_window_grad(const SsimWindow& win, const SsimBwdLds& s, int py, int px, float& va, float& vb,
                                                     float& wa, float& wb) {
    constexpr int NM = SsimBwdMaps<WA, WB>::NM, MA = SsimBwdMaps<WA, WB>::MA, MB = SsimBwdMaps<WA, WB>::MB;
    float tq[NM];
#pragma unroll
    for (int q = 0; q < NM; ++q) tq[q] = 0.f;
#pragma unroll
    for (int k = 0; k < SSIM_WIN; ++k) {
        const float w = win.w[k];
#pragma unroll
        for (int q = 0; q < NM; ++q) tq[q] = fmaf(w, s.hm[q * (SSIM_SH * SSIM_TW) + (py + k) * SSIM_TW + px], tq[q]);
    }
    va = s.sa[(py + SSIM_APRON) * SSIM_BW + px + SSIM_APRON];
    vb = s.sb[(py + SSIM_APRON) * SSIM_BW + px + SSIM_APRON];
    if (WA) wa = fmaf(vb, tq[1], fmaf(2.f * va, tq[0], tq[MA]));
    if (WB) wb = fmaf(va, tq[1], fmaf(2.f * vb, tq[0], tq[MB]));
}

// the tile's pixels: thread = pixel column px, pixel rows py and py + SSIM_TH / 2.  pixel(py, px, y, x, off, ga, gb) is called for
// a pixel inside the view ((y, x): view coordinates, off: its element of the first plane) and adds to (ga, gb) = 0; outside the
// view the gradient is 0.  Under luma the three channel gradients are the luma gradient times the channel's coefficient
template <bool WA, bool WB, typename Pixel>
__device__ __forceinline__ void ssim_bwd_pixels(const SsimGeom& g, const SsimBwdTile& t, float* __restrict__ da, float* __restrict__ db,
                                                Pixel pixel) {
    const int px = threadIdx.x & (SSIM_TW - 1);
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int py = (threadIdx.x / SSIM_TW) + half * (SSIM_TH / 2);
        const int y = t.cy0 + py, x = t.cx0 + px;                     // view coordinates
        if (y + g.crop >= g.H || x + g.crop >= g.W) continue;         // past the image (ragged last tiles)
        const int64_t off = t.base + (int64_t)(y + g.crop) * g.W + (x + g.crop), pe = t.plane_elems;
        float ga = 0.f, gb = 0.f;
        if (y >= 0 && y < g.Hc && x >= 0 && x < g.Wc) pixel(py, px, y, x, off, ga, gb);
        if (g.luma) {
            if (WA) { da[off] = 0.299f * ga; da[off + pe] = 0.587f * ga; da[off + 2 * pe] = 0.114f * ga; }
            if (WB) { db[off] = 0.299f * gb; db[off + pe] = 0.587f * gb; db[off + 2 * pe] = 0.114f * gb; }
        } else {
            if (WA) da[off] = ga;
            if (WB) db[off] = gb;
        }
    }
}

// host: launch(wa, wb) with the two std::bool_constant of "da wanted", "db wanted" (one of them is)
template <typename Launch>
static void ssim_bwd_dispatch(const float* da, const float* db, Launch launch) {
    if (da && db) launch(std::true_type{}, std::true_type{});
    else if (da) launch(std::true_type{}, std::false_type{});
    else launch(std::false_type{}, std::true_type{});
}
