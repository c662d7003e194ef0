// image_loss.hip -- one image-space training loss of two fp32 NCHW batches, forward and backward, entirely on the device:
//   loss[n] = w_ssim (1 - SSIM[n]) + w_pix mean_{C',H',W'} rho(a - b),   rho(d) = |d| / sqrt(d^2 + eps^2) / d^2
// on the view of sisr_ssim.h (`crop` pixels stripped from every side, BT.601 luma for C == 3 with `luma`), SSIM exactly the metric's
// (11 x 11 separable Gaussian, sigma 1.5, "valid" positions, C1 = (0.01 L)^2, C2 = (0.03 L)^2).  Nothing here synchronises with the
// host, nothing uses atomics, every sum has a fixed order: the same bits every call, and the launches can sit inside a captured step.
//
// Forward: ssim_tile_kernel of sisr_ssim.h, the kernel of the metric, instantiated per pixel term ('mse' with the SSIM term IS the
// metric's instantiation) and with apron 10 or, without the SSIM term, 0.  The `ssim` of return_parts is therefore metrics.ssim bit
// for bit.  image_loss_finish_kernel folds an image's partials in a fixed order in double (ssim_fold_image) and weighs the terms.
//
// Backward: one launch in gather form, nothing saved by the forward but the inputs.  Per window position q with moments mu_a, mu_b,
// E_aa, E_bb, E_ab:  A1 = 2 mu_a mu_b + C1, A2 = 2 (E_ab - mu_a mu_b) + C2, B1 = mu_a^2 + mu_b^2 + C1,
// B2 = (E_aa - mu_a^2) + (E_bb - mu_b^2) + C2, S = A1 A2 / (B1 B2), and
//   D_e = dS/dE_ab = 2 A1 / (B1 B2),   D_q = dS/dE_aa = dS/dE_bb = -S / B2,
//   D_mua = 2 mu_b (A2 - A1) / (B1 B2) + 2 mu_a S (1 / B2 - 1 / B1),   D_mub: mu_a and mu_b exchanged.
// With T the transposed window (the same symmetric taps over a map that is zero outside the valid positions):
//   d(sum_q S)/da(p) = T(D_mua)(p) + 2 a(p) T(D_q)(p) + b(p) T(D_e)(p),   db: a and b exchanged.
// A workgroup owns an SSIM_TH x SSIM_TW tile of pixels of one (image, plane) of the WHOLE image (so the cropped border is written
// too: exact zeros).  It stages the (SSIM_TH + 20) x (SSIM_TW + 20) pixels around the tile, recomputes the moments at the
// (SSIM_TH + 10) x (SSIM_TW + 10) positions whose windows touch the tile, leaves the derivative maps in LDS, filters them separably
// and adds the pixel term.  Under luma it writes all three channel gradients (the luma gradient times the channel's coefficient).
// LDS: 2 x 36 x 52 staged pixels (15.0 KB) + 5 x 36 x 42 row-filtered moments (30.2 KB, reused for the row-filtered derivative
// maps) + 4 x 26 x 42 derivative maps (17.5 KB) = 62,688 B per workgroup.

// the forward comes from this header under the compiler's default contraction, as metrics.hip compiles it: it has to stay ABOVE the
// pragma below, or the forward's SSIM would no longer be the metric's bits
#include "sisr_ssim.h"

// every product and sum below is rounded as written (fused multiply-adds are spelled fmaf): the three instantiations of the backward
// kernel then compute a gradient with the same instructions, so da is the same bits whether or not db is asked for
#pragma clang fp contract(off)

#define IL_BH (SSIM_TH + 2 * SSIM_APRON)      // backward: staged pixels
#define IL_BW (SSIM_TW + 2 * SSIM_APRON)
#define IL_PIX_NONE (-1)                      // internal: w_pix == 0, the pixel term contributes no gradient

// one pixel of the view; off: the element of the first plane
__device__ __forceinline__ float il_load(const float* __restrict__ p, int64_t off, int64_t plane_elems, int luma) {
    return luma ? fmaf(0.114f, p[off + 2 * plane_elems], fmaf(0.587f, p[off + plane_elems], 0.299f * p[off])) : p[off];
}

// rho'(d); L1: 0 at d == 0 (torch's sign)
__device__ __forceinline__ float il_rho_grad(float d, int kind, float eps2) {
    if (kind == SISR_PIX_L1) return d > 0.f ? 1.f : d < 0.f ? -1.f : 0.f;
    if (kind == SISR_PIX_CHARBONNIER) return d / sqrtf(fmaf(d, d, eps2));
    return kind == SISR_PIX_MSE ? 2.f * d : 0.f;
}

// the five moments of one staged row at window column 0: p points at the first of SSIM_WIN consecutive pixels
__device__ __forceinline__ void il_row_moments(const SsimWindow& win, const float* pa, const float* pb, float (&m)[5]) {
    float ma = 0.f, mb = 0.f, maa = 0.f, mbb = 0.f, mab = 0.f;
#pragma unroll
    for (int k = 0; k < SSIM_WIN; ++k) {
        const float w = win.w[k], u = pa[k], v = pb[k];
        const float wu = w * u, wv = w * v;
        ma += wu; mb += wv;
        maa = fmaf(wu, u, maa); mbb = fmaf(wv, v, mbb); mab = fmaf(wu, v, mab);
    }
    m[0] = ma; m[1] = mb; m[2] = maa; m[3] = mbb; m[4] = mab;
}

// one workgroup per image: the image's partials folded in double (ssim_fold_image)
__global__ void __launch_bounds__(SISR_BLOCK) image_loss_finish_kernel(const float* __restrict__ part, int per_image, int with_ssim,
                                                                       double n_ssim, double n_pix, double w_ssim, double w_pix,
                                                                       float* __restrict__ loss, float* __restrict__ ssim,
                                                                       float* __restrict__ pix) {
    double s[2];
    ssim_fold_image(part, per_image, s);
    if (threadIdx.x == 0) {
        const double mean_pix = s[1] / n_pix;
        double l = w_pix * mean_pix;
        if (with_ssim) {
            const double mean_ssim = s[0] / n_ssim;
            l += w_ssim * (1.0 - mean_ssim);
            if (ssim) ssim[blockIdx.x] = (float)mean_ssim;
        }
        loss[blockIdx.x] = (float)l;
        if (pix) pix[blockIdx.x] = (float)mean_pix;
    }
}

// workgroup = (image n, plane, pixel-tile row, pixel-tile column) of the WHOLE image, flat in that order.  WA / WB: da / db wanted.
// ks = -w_ssim / (C' Hv Wv), kp = w_pix / (C' H' W'): the factors of the two terms in front of the upstream gradient g[n]
template <bool WA, bool WB>
__global__ void __launch_bounds__(SISR_BLOCK) image_loss_bwd_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                    const float* __restrict__ gup, SsimGeom g,
                                                                    SsimWindow win, float c1, float c2, int pix_kind,
                                                                    float eps2, float ks, float kp, float* __restrict__ da,
                                                                    float* __restrict__ db) {
    constexpr int NM = 2 + (WA ? 1 : 0) + (WB ? 1 : 0);              // derivative maps: D_q, D_e, D_mua and / or D_mub
    constexpr int MA = 2, MB = WA ? 3 : 2;                           // indices of D_mua / D_mub
    __shared__ float sa[IL_BH * IL_BW], sb[IL_BH * IL_BW];
    __shared__ float hm[5 * IL_BH * SSIM_SW];                          // row-filtered moments [5][IL_BH][SSIM_SW], then maps [NM][SSIM_SH][SSIM_TW]
    __shared__ float dm[4][SSIM_SH * SSIM_SW];
    static_assert(4 * SSIM_SH * SSIM_TW <= 5 * IL_BH * SSIM_SW, "the row-filtered derivative maps reuse the moments' LDS");
    const int tid = threadIdx.x;
    const int tiles = g.btiles_y * g.btiles_x, per_image = g.planes * tiles;
    const int n = blockIdx.x / per_image, r = blockIdx.x - n * per_image;
    const int plane = r / tiles, t = r - plane * tiles;
    const int ty = t / g.btiles_x, tx = t - ty * g.btiles_x;
    const int cy0 = ty * SSIM_TH - g.crop, cx0 = tx * SSIM_TW - g.crop;   // tile origin in the view's coordinates (< 0 in the border)
    const int64_t plane_elems = (int64_t)g.H * g.W;
    const int64_t base = ((int64_t)n * g.C + (g.luma ? 0 : plane)) * plane_elems;
    const float gn = gup[n];
    const float ksn = gn * ks, kpn = gn * kp;
    if (g.apron) {
        // the pixels under every window that touches the tile; outside the view: zeros
        for (int i = tid; i < IL_BH * IL_BW; i += SISR_BLOCK) {
            const int ly = i / IL_BW, lx = i - ly * IL_BW;
            const int y = cy0 - SSIM_APRON + ly, x = cx0 - SSIM_APRON + lx;
            float va = 0.f, vb = 0.f;
            if (y >= 0 && y < g.Hc && x >= 0 && x < g.Wc) {
                const int64_t off = base + (int64_t)(y + g.crop) * g.W + (x + g.crop);
                va = il_load(a, off, plane_elems, g.luma);
                vb = il_load(b, off, plane_elems, g.luma);
            }
            sa[i] = va;
            sb[i] = vb;
        }
        __syncthreads();
        // horizontal pass: every staged row at the SSIM_SW position columns (lanes on consecutive columns)
        for (int i = tid; i < IL_BH * SSIM_SW; i += SISR_BLOCK) {
            const int ly = i / SSIM_SW, ox = i - ly * SSIM_SW;
            float m[5];
            il_row_moments(win, sa + ly * IL_BW + ox, sb + ly * IL_BW + ox, m);
#pragma unroll
            for (int q = 0; q < 5; ++q) hm[q * (IL_BH * SSIM_SW) + i] = m[q];
        }
        __syncthreads();
        // vertical pass + derivative maps at the SSIM_SH x SSIM_SW positions (position (qy, qx) = view position
        // (cy0 - 10 + qy, cx0 - 10 + qx)); i + k SSIM_SW: lanes on consecutive addresses
        for (int i = tid; i < SSIM_SH * SSIM_SW; i += SISR_BLOCK) {
            const int qy = i / SSIM_SW, qx = i - qy * SSIM_SW;
            float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < SSIM_WIN; ++k) {
                const float w = win.w[k];
#pragma unroll
                for (int q = 0; q < 5; ++q) m[q] = fmaf(w, hm[q * (IL_BH * SSIM_SW) + i + k * SSIM_SW], m[q]);
            }
            const int py = cy0 - SSIM_APRON + qy, px = cx0 - SSIM_APRON + qx;
            const bool valid = py >= 0 && py < g.Hv && px >= 0 && px < g.Wv;
            const float mu_aa = m[0] * m[0], mu_bb = m[1] * m[1], mu_ab = m[0] * m[1];
            const float a1 = fmaf(2.f, mu_ab, c1), a2 = fmaf(2.f, m[4] - mu_ab, c2);
            const float rb1 = 1.f / (mu_aa + mu_bb + c1), rb2 = 1.f / ((m[2] - mu_aa) + (m[3] - mu_bb) + c2);
            const float r12 = rb1 * rb2;
            const float s = a1 * a2 * r12;
            const float cross = 2.f * (a2 - a1) * r12, self = 2.f * s * (rb2 - rb1);
            dm[0][i] = valid ? -s * rb2 : 0.f;
            dm[1][i] = valid ? 2.f * a1 * r12 : 0.f;
            if (WA) dm[MA][i] = valid ? fmaf(m[1], cross, m[0] * self) : 0.f;
            if (WB) dm[MB][i] = valid ? fmaf(m[0], cross, m[1] * self) : 0.f;
        }
        __syncthreads();
        // transposed window, horizontal: pixel column px of the tile gathers positions px .. px + 10 (symmetric taps)
        for (int i = tid; i < SSIM_SH * SSIM_TW; i += SISR_BLOCK) {
            const int qy = i / SSIM_TW, px = i - qy * SSIM_TW;
            float h[NM];
#pragma unroll
            for (int q = 0; q < NM; ++q) h[q] = 0.f;
#pragma unroll
            for (int k = 0; k < SSIM_WIN; ++k) {
                const float w = win.w[k];
#pragma unroll
                for (int q = 0; q < NM; ++q) h[q] = fmaf(w, dm[q][qy * SSIM_SW + px + k], h[q]);
            }
#pragma unroll
            for (int q = 0; q < NM; ++q) hm[q * (SSIM_SH * SSIM_TW) + i] = h[q];
        }
        __syncthreads();
    }
    // vertical + the pixel term + store: thread = pixel column px, pixel rows py and py + SSIM_TH / 2
    const int px = tid & (SSIM_TW - 1);
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int py = (tid / SSIM_TW) + half * (SSIM_TH / 2);
        const int y = cy0 + py, x = cx0 + px;                         // view coordinates
        if (y + g.crop >= g.H || x + g.crop >= g.W) continue;         // past the image (ragged last tiles)
        const bool inside = y >= 0 && y < g.Hc && x >= 0 && x < g.Wc;
        const int64_t off = base + (int64_t)(y + g.crop) * g.W + (x + g.crop);
        float ga = 0.f, gb = 0.f;
        if (inside) {
            float va, vb;
            if (g.apron) {
                float tq[NM];
#pragma unroll
                for (int q = 0; q < NM; ++q) tq[q] = 0.f;
#pragma unroll
                for (int k = 0; k < SSIM_WIN; ++k) {
                    const float w = win.w[k];
#pragma unroll
                    for (int q = 0; q < NM; ++q) tq[q] = fmaf(w, hm[q * (SSIM_SH * SSIM_TW) + (py + k) * SSIM_TW + px], tq[q]);
                }
                va = sa[(py + SSIM_APRON) * IL_BW + px + SSIM_APRON];
                vb = sb[(py + SSIM_APRON) * IL_BW + px + SSIM_APRON];
                if (WA) ga = ksn * fmaf(vb, tq[1], fmaf(2.f * va, tq[0], tq[MA]));
                if (WB) gb = ksn * fmaf(va, tq[1], fmaf(2.f * vb, tq[0], tq[MB]));
            } else {
                va = il_load(a, off, plane_elems, g.luma);
                vb = il_load(b, off, plane_elems, g.luma);
            }
            const float dp = kpn * il_rho_grad(va - vb, pix_kind, eps2);
            ga += dp;
            gb -= dp;
        }
        if (g.luma) {
            if (WA) { da[off] = 0.299f * ga; da[off + plane_elems] = 0.587f * ga; da[off + 2 * plane_elems] = 0.114f * ga; }
            if (WB) { db[off] = 0.299f * gb; db[off + plane_elems] = 0.587f * gb; db[off + 2 * plane_elems] = 0.114f * gb; }
        } else {
            if (WA) da[off] = ga;
            if (WB) db[off] = gb;
        }
    }
}

extern "C" int sisr_image_loss_ws_floats(int32_t N, int32_t C, int32_t H, int32_t W, int32_t crop, int32_t luma,
                                         int32_t with_ssim) {
    return ssim_ws_floats(N, C, H, W, crop, luma, with_ssim != 0 ? SSIM_APRON : 0);
}

static bool image_loss_scalars_ok(float data_range, int pix_kind, float eps) {
    return data_range > 0.f && eps >= 0.f && pix_kind >= SISR_PIX_L1 && pix_kind <= SISR_PIX_MSE;      // (a NaN fails both comparisons)
}

extern "C" int sisr_image_loss_fwd(const float* a, const float* b, int32_t N, int32_t C, int32_t H, int32_t W, int32_t crop,
                                   int32_t luma, float data_range, float w_ssim, float w_pix, int32_t pix_kind, float eps,
                                   float* work, float* loss, float* ssim, float* pix, void* stream) {
    const int with_ssim = (w_ssim != 0.f || ssim != nullptr) ? 1 : 0;
    const int ws = sisr_image_loss_ws_floats(N, C, H, W, crop, luma, with_ssim);
    if (ws < 0) return ws;
    if (!a || !b || !work || !loss || !image_loss_scalars_ok(data_range, pix_kind, eps)) return SISR_E_BADARG;
    SsimGeom g;
    ssim_geom(C, H, W, crop, luma, with_ssim ? SSIM_APRON : 0, g);
    hipStream_t st = sisr_stream(stream);
#define IL_FWD_LAUNCH(PIX)                                                                                                       \
    (with_ssim ? ssim_launch_tiles<PIX, SSIM_APRON>(ws, st, a, b, g, (double)data_range, 1, eps * eps, work)                       \
               : ssim_launch_tiles<PIX, 0>(ws, st, a, b, g, (double)data_range, 0, eps * eps, work))
    const int e = pix_kind == SISR_PIX_L1            ? IL_FWD_LAUNCH(SISR_PIX_L1)
                  : pix_kind == SISR_PIX_CHARBONNIER ? IL_FWD_LAUNCH(SISR_PIX_CHARBONNIER)
                                                     : IL_FWD_LAUNCH(SISR_PIX_MSE);
#undef IL_FWD_LAUNCH
    if (e) return e;
    hipLaunchKernelGGL(image_loss_finish_kernel, dim3((unsigned)N), dim3(SISR_BLOCK), 0, st, (const float*)work,
                       g.planes * g.tiles_y * g.tiles_x, with_ssim, (double)g.planes * g.Hv * g.Wv,
                       (double)g.planes * g.Hc * g.Wc, (double)w_ssim, (double)w_pix, loss, ssim, pix);
    SISR_CHECK_LAUNCH();
    return 0;
}

extern "C" int sisr_image_loss_bwd(const float* a, const float* b, const float* gup, int32_t N, int32_t C, int32_t H, int32_t W,
                                   int32_t crop, int32_t luma, float data_range, float w_ssim, float w_pix, int32_t pix_kind,
                                   float eps, float* da, float* db, void* stream) {
    const int with_ssim = w_ssim != 0.f ? 1 : 0;
    SsimGeom g;
    if (N <= 0) return SISR_E_BADARG;
    if (!ssim_geom(C, H, W, crop, luma, with_ssim ? SSIM_APRON : 0, g)) return (C != 1 && C != 3) ? SISR_E_UNSUPPORTED : SISR_E_BADARG;
    if (!a || !b || !gup || (!da && !db) || !image_loss_scalars_ok(data_range, pix_kind, eps)) return SISR_E_BADARG;
    const int64_t wgs = (int64_t)N * g.planes * g.btiles_y * g.btiles_x;
    if (wgs > INT32_MAX) return SISR_E_TOOBIG;
    const double L = (double)data_range;
    const float c1 = (float)(0.01 * L * 0.01 * L), c2 = (float)(0.03 * L * 0.03 * L);
    const float ks = with_ssim ? (float)(-(double)w_ssim / ((double)g.planes * g.Hv * g.Wv)) : 0.f;
    const float kp = (float)((double)w_pix / ((double)g.planes * g.Hc * g.Wc));
    const int kind = w_pix != 0.f ? (int)pix_kind : IL_PIX_NONE;
    const SsimWindow win = ssim_window();
    hipStream_t st = sisr_stream(stream);
#define IL_BWD_LAUNCH(WA, WB)                                                                                                  \
    hipLaunchKernelGGL((image_loss_bwd_kernel<WA, WB>), dim3((unsigned)wgs), dim3(SISR_BLOCK), 0, st, a, b, gup, g, win, c1, c2, \
                       kind, eps * eps, ks, kp, da, db)
    if (da && db) IL_BWD_LAUNCH(true, true);
    else if (da) IL_BWD_LAUNCH(true, false);
    else IL_BWD_LAUNCH(false, true);
#undef IL_BWD_LAUNCH
    SISR_CHECK_LAUNCH();
    return 0;
}
