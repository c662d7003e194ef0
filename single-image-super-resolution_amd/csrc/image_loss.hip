// image_loss.hip -- one image-space training loss of two fp32 NCHW batches, forward and backward, entirely on the device:
//   loss[n] = w_ssim (1 - SSIM[n]) + w_pix mean_{C',H',W'} rho(a - b),   rho(d) = |d| / sqrt(d^2 + eps^2) / d^2
// on the view of metrics.hip (`crop` pixels stripped from every side, BT.601 luma for C == 3 with `luma`), SSIM exactly the metric's
// (11 x 11 separable Gaussian, sigma 1.5, "valid" positions, C1 = (0.01 L)^2, C2 = (0.03 L)^2).  Nothing here synchronises with the
// host, nothing uses atomics, every sum has a fixed order: the same bits every call, and the launches can sit inside a captured step.
//
// Forward: the tile scheme of metrics_tile_kernel (a kernel of its own, so that the metric keeps its arithmetic bit for bit).  One
// workgroup per IL_TH x IL_TW tile of window positions stages the (IL_TH + 10) x (IL_TW + 10) pixels under them into LDS once,
// filters the five moments horizontally into LDS and vertically from it and leaves ONE partial (sum of SSIM values, sum of rho);
// the rho sum rides on the staging pass, the tiles of the last row / column also taking the 10 pixels behind them.  Without the
// SSIM term the apron is 0: the grid partitions the view itself into IL_TH x IL_TW pixel tiles and nothing goes through LDS.
// image_loss_finish_kernel folds an image's partials in a fixed order in double.
//
// Backward: one launch in gather form, nothing saved by the forward but the inputs.  Per window position q with moments mu_a, mu_b,
// E_aa, E_bb, E_ab:  A1 = 2 mu_a mu_b + C1, A2 = 2 (E_ab - mu_a mu_b) + C2, B1 = mu_a^2 + mu_b^2 + C1,
// B2 = (E_aa - mu_a^2) + (E_bb - mu_b^2) + C2, S = A1 A2 / (B1 B2), and
//   D_e = dS/dE_ab = 2 A1 / (B1 B2),   D_q = dS/dE_aa = dS/dE_bb = -S / B2,
//   D_mua = 2 mu_b (A2 - A1) / (B1 B2) + 2 mu_a S (1 / B2 - 1 / B1),   D_mub: mu_a and mu_b exchanged.
// With T the transposed window (the same symmetric taps over a map that is zero outside the valid positions):
//   d(sum_q S)/da(p) = T(D_mua)(p) + 2 a(p) T(D_q)(p) + b(p) T(D_e)(p),   db: a and b exchanged.
// A workgroup owns an IL_TH x IL_TW tile of pixels of one (image, plane) of the WHOLE image (so the cropped border is written too:
// exact zeros).  It stages the (IL_TH + 20) x (IL_TW + 20) pixels around the tile, recomputes the moments at the
// (IL_TH + 10) x (IL_TW + 10) positions whose windows touch the tile, leaves the derivative maps in LDS, filters them separably and
// adds the pixel term.  Under luma it writes all three channel gradients (the luma gradient times the channel's coefficient).
// LDS: 2 x 36 x 52 staged pixels (15.0 KB) + 5 x 36 x 42 row-filtered moments (30.2 KB, reused for the row-filtered derivative
// maps) + 4 x 26 x 42 derivative maps (17.5 KB) = 62,688 B per workgroup.
#include "sisr_dev.h"

#include <cmath>

// every product and sum below is rounded as written (fused multiply-adds are spelled fmaf): the three instantiations of the backward
// kernel then compute a gradient with the same instructions, so da is the same bits whether or not db is asked for
#pragma clang fp contract(off)

#define IL_WIN 11
#define IL_APRON (IL_WIN - 1)
#define IL_TH 16
#define IL_TW 32
#define IL_SH (IL_TH + IL_APRON)              // forward: staged pixels; backward: window positions that touch a pixel tile
#define IL_SW (IL_TW + IL_APRON)
#define IL_BH (IL_TH + 2 * IL_APRON)          // backward: staged pixels
#define IL_BW (IL_TW + 2 * IL_APRON)
#define IL_PIX_NONE (-1)                      // internal: w_pix == 0, the pixel term contributes no gradient
static_assert(IL_TH * IL_TW == 2 * SISR_BLOCK, "the last pass gives every thread two pixels / window positions");

struct ImageLossWindow { float w[IL_WIN]; };

struct ImageLossGeom {
    int C, H, W, crop, luma, with_ssim;
    int Hc, Wc;                  // the view
    int Hv, Wv;                  // window positions (with_ssim)
    int planes;                  // C'
    int tiles_y, tiles_x;        // forward grid: over window positions (with_ssim) or over the view's pixels
    int btiles_y, btiles_x;      // backward grid: over the whole image's pixels
};

// false: the shapes are outside what the kernels take
static bool image_loss_geom(int C, int H, int W, int crop, int luma, int with_ssim, ImageLossGeom& g) {
    if ((C != 1 && C != 3) || crop < 0 || H <= 0 || W <= 0) return false;
    g.C = C; g.H = H; g.W = W; g.crop = crop;
    g.luma = (luma != 0 && C == 3) ? 1 : 0;
    g.with_ssim = with_ssim != 0 ? 1 : 0;
    const int64_t hc = (int64_t)H - 2 * (int64_t)crop, wc = (int64_t)W - 2 * (int64_t)crop;
    const int least = g.with_ssim ? IL_WIN : 1;
    if (hc < least || wc < least) return false;
    g.Hc = (int)hc; g.Wc = (int)wc;
    g.Hv = g.Hc - IL_APRON; g.Wv = g.Wc - IL_APRON;
    g.planes = g.luma ? 1 : C;
    const int fh = g.with_ssim ? g.Hv : g.Hc, fw = g.with_ssim ? g.Wv : g.Wc;
    g.tiles_y = (fh + IL_TH - 1) / IL_TH;
    g.tiles_x = (fw + IL_TW - 1) / IL_TW;
    g.btiles_y = (H + IL_TH - 1) / IL_TH;
    g.btiles_x = (W + IL_TW - 1) / IL_TW;
    return true;
}

// the 11-tap Gaussian, sigma 1.5, normalised in double (the metric's window)
static ImageLossWindow image_loss_window() {
    ImageLossWindow win;
    double wd[IL_WIN], sum = 0.0;
    for (int k = 0; k < IL_WIN; ++k) {
        const double d = (double)(k - IL_WIN / 2);
        wd[k] = exp(-d * d / (2.0 * 1.5 * 1.5));
        sum += wd[k];
    }
    for (int k = 0; k < IL_WIN; ++k) win.w[k] = (float)(wd[k] / sum);
    return win;
}

// one pixel of the view; off: the element of the first plane
__device__ __forceinline__ float il_load(const float* __restrict__ p, int64_t off, int64_t plane_elems, int luma) {
    return luma ? fmaf(0.114f, p[off + 2 * plane_elems], fmaf(0.587f, p[off + plane_elems], 0.299f * p[off])) : p[off];
}

__device__ __forceinline__ float il_rho(float d, int kind, float eps2) {
    return kind == SISR_PIX_L1 ? fabsf(d) : kind == SISR_PIX_CHARBONNIER ? sqrtf(fmaf(d, d, eps2)) : d * d;
}

// rho'(d); L1: 0 at d == 0 (torch's sign)
__device__ __forceinline__ float il_rho_grad(float d, int kind, float eps2) {
    if (kind == SISR_PIX_L1) return d > 0.f ? 1.f : d < 0.f ? -1.f : 0.f;
    if (kind == SISR_PIX_CHARBONNIER) return d / sqrtf(fmaf(d, d, eps2));
    return kind == SISR_PIX_MSE ? 2.f * d : 0.f;
}

// the five moments of one staged row at window column 0: p points at the first of IL_WIN consecutive pixels
__device__ __forceinline__ void il_row_moments(const ImageLossWindow& win, const float* pa, const float* pb, float (&m)[5]) {
    float ma = 0.f, mb = 0.f, maa = 0.f, mbb = 0.f, mab = 0.f;
#pragma unroll
    for (int k = 0; k < IL_WIN; ++k) {
        const float w = win.w[k], u = pa[k], v = pb[k];
        const float wu = w * u, wv = w * v;
        ma += wu; mb += wv;
        maa = fmaf(wu, u, maa); mbb = fmaf(wv, v, mbb); mab = fmaf(wu, v, mab);
    }
    m[0] = ma; m[1] = mb; m[2] = maa; m[3] = mbb; m[4] = mab;
}

// workgroup = (image n, plane, tile row, tile column), flat in that order; part[workgroup][2] = (sum of SSIM values, sum of rho)
__global__ void __launch_bounds__(SISR_BLOCK) image_loss_tile_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                     ImageLossGeom g, ImageLossWindow win, float c1, float c2,
                                                                     int pix_kind, float eps2, float* __restrict__ part) {
    __shared__ float sa[IL_SH * IL_SW], sb[IL_SH * IL_SW];
    __shared__ float hm[5][IL_SH * IL_TW];
    const int tid = threadIdx.x;
    const int tiles = g.tiles_y * g.tiles_x, per_image = g.planes * tiles;
    const int n = blockIdx.x / per_image, r = blockIdx.x - n * per_image;
    const int plane = r / tiles, t = r - plane * tiles;
    const int ty = t / g.tiles_x, tx = t - ty * g.tiles_x;
    const int y0 = ty * IL_TH, x0 = tx * IL_TW;                       // tile origin in the view
    // staged block: the tile plus the apron under its windows (none without SSIM); pixels this workgroup counts for the pixel
    // term: its IL_TH x IL_TW block, and everything behind it in the last row / column
    const int apron = g.with_ssim ? IL_APRON : 0;
    const int sh = IL_TH + apron, sw = IL_TW + apron;
    const int own_h = ty == g.tiles_y - 1 ? sh : IL_TH, own_w = tx == g.tiles_x - 1 ? sw : IL_TW;
    const int64_t plane_elems = (int64_t)g.H * g.W;
    const int64_t base = ((int64_t)n * g.C + (g.luma ? 0 : plane)) * plane_elems;
    float ss_px[2] = {0.f, 0.f};          // sum of SSIM values, sum of rho
    float &ss = ss_px[0], &px = ss_px[1];
    for (int i = tid; i < sh * sw; i += SISR_BLOCK) {
        const int ly = i / sw, lx = i - ly * sw;
        const int y = y0 + ly, x = x0 + lx;
        float va = 0.f, vb = 0.f;
        if (y < g.Hc && x < g.Wc) {
            const int64_t off = base + (int64_t)(y + g.crop) * g.W + (x + g.crop);
            va = il_load(a, off, plane_elems, g.luma);
            vb = il_load(b, off, plane_elems, g.luma);
            if (ly < own_h && lx < own_w) px += il_rho(va - vb, pix_kind, eps2);
        }
        if (g.with_ssim) {                // (sw == IL_SW)
            sa[i] = va;
            sb[i] = vb;
        }
    }
    if (g.with_ssim) {
        __syncthreads();
        // horizontal pass: every staged row, IL_TW window columns (lanes on consecutive columns: conflict-free LDS reads)
        for (int i = tid; i < IL_SH * IL_TW; i += SISR_BLOCK) {
            const int ly = i / IL_TW, ox = i - ly * IL_TW;
            float m[5];
            il_row_moments(win, sa + ly * IL_SW + ox, sb + ly * IL_SW + ox, m);
#pragma unroll
            for (int q = 0; q < 5; ++q) hm[q][i] = m[q];
        }
        __syncthreads();
        // vertical pass + SSIM map: thread = window column ox, window rows oy and oy + IL_TH / 2
        const int ox = tid & (IL_TW - 1);
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const int oy = (tid / IL_TW) + half * (IL_TH / 2);
            float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < IL_WIN; ++k) {
                const float w = win.w[k];
#pragma unroll
                for (int q = 0; q < 5; ++q) m[q] = fmaf(w, hm[q][(oy + k) * IL_TW + ox], m[q]);
            }
            if (y0 + oy < g.Hv && x0 + ox < g.Wv) {
                const float mu_aa = m[0] * m[0], mu_bb = m[1] * m[1], mu_ab = m[0] * m[1];
                const float var_a = m[2] - mu_aa, var_b = m[3] - mu_bb, cov = m[4] - mu_ab;
                ss += ((2.f * mu_ab + c1) * (2.f * cov + c2)) / ((mu_aa + mu_bb + c1) * (var_a + var_b + c2));
            }
        }
    }
    block_partial_sum(ss_px);
    if (tid == 0) {
        part[2 * (int64_t)blockIdx.x] = ss;
        part[2 * (int64_t)blockIdx.x + 1] = px;
    }
}

// one workgroup per image: the image's partials added in a fixed order in double (fold_partials_double)
__global__ void __launch_bounds__(SISR_BLOCK) image_loss_finish_kernel(const float* __restrict__ part, int per_image, int with_ssim,
                                                                       double n_ssim, double n_pix, double w_ssim, double w_pix,
                                                                       float* __restrict__ loss, float* __restrict__ ssim,
                                                                       float* __restrict__ pix) {
    const float* p = part + 2 * (int64_t)blockIdx.x * per_image;
    double s[2];
    fold_partials_double(per_image, s, [&](int64_t i, double* acc) { acc[0] += (double)p[2 * i]; acc[1] += (double)p[2 * i + 1]; });
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
                                                                    const float* __restrict__ gup, ImageLossGeom g,
                                                                    ImageLossWindow win, float c1, float c2, int pix_kind,
                                                                    float eps2, float ks, float kp, float* __restrict__ da,
                                                                    float* __restrict__ db) {
    constexpr int NM = 2 + (WA ? 1 : 0) + (WB ? 1 : 0);              // derivative maps: D_q, D_e, D_mua and / or D_mub
    constexpr int MA = 2, MB = WA ? 3 : 2;                           // indices of D_mua / D_mub
    __shared__ float sa[IL_BH * IL_BW], sb[IL_BH * IL_BW];
    __shared__ float hm[5 * IL_BH * IL_SW];                          // row-filtered moments [5][IL_BH][IL_SW], then maps [NM][IL_SH][IL_TW]
    __shared__ float dm[4][IL_SH * IL_SW];
    static_assert(4 * IL_SH * IL_TW <= 5 * IL_BH * IL_SW, "the row-filtered derivative maps reuse the moments' LDS");
    const int tid = threadIdx.x;
    const int tiles = g.btiles_y * g.btiles_x, per_image = g.planes * tiles;
    const int n = blockIdx.x / per_image, r = blockIdx.x - n * per_image;
    const int plane = r / tiles, t = r - plane * tiles;
    const int ty = t / g.btiles_x, tx = t - ty * g.btiles_x;
    const int cy0 = ty * IL_TH - g.crop, cx0 = tx * IL_TW - g.crop;   // tile origin in the view's coordinates (< 0 in the border)
    const int64_t plane_elems = (int64_t)g.H * g.W;
    const int64_t base = ((int64_t)n * g.C + (g.luma ? 0 : plane)) * plane_elems;
    const float gn = gup[n];
    const float ksn = gn * ks, kpn = gn * kp;
    if (g.with_ssim) {
        // the pixels under every window that touches the tile; outside the view: zeros
        for (int i = tid; i < IL_BH * IL_BW; i += SISR_BLOCK) {
            const int ly = i / IL_BW, lx = i - ly * IL_BW;
            const int y = cy0 - IL_APRON + ly, x = cx0 - IL_APRON + lx;
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
        // horizontal pass: every staged row at the IL_SW position columns (lanes on consecutive columns)
        for (int i = tid; i < IL_BH * IL_SW; i += SISR_BLOCK) {
            const int ly = i / IL_SW, ox = i - ly * IL_SW;
            float m[5];
            il_row_moments(win, sa + ly * IL_BW + ox, sb + ly * IL_BW + ox, m);
#pragma unroll
            for (int q = 0; q < 5; ++q) hm[q * (IL_BH * IL_SW) + i] = m[q];
        }
        __syncthreads();
        // vertical pass + derivative maps at the IL_SH x IL_SW positions (position (qy, qx) = view position
        // (cy0 - 10 + qy, cx0 - 10 + qx)); i + k IL_SW: lanes on consecutive addresses
        for (int i = tid; i < IL_SH * IL_SW; i += SISR_BLOCK) {
            const int qy = i / IL_SW, qx = i - qy * IL_SW;
            float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < IL_WIN; ++k) {
                const float w = win.w[k];
#pragma unroll
                for (int q = 0; q < 5; ++q) m[q] = fmaf(w, hm[q * (IL_BH * IL_SW) + i + k * IL_SW], m[q]);
            }
            const int py = cy0 - IL_APRON + qy, px = cx0 - IL_APRON + qx;
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
        for (int i = tid; i < IL_SH * IL_TW; i += SISR_BLOCK) {
            const int qy = i / IL_TW, px = i - qy * IL_TW;
            float h[NM];
#pragma unroll
            for (int q = 0; q < NM; ++q) h[q] = 0.f;
#pragma unroll
            for (int k = 0; k < IL_WIN; ++k) {
                const float w = win.w[k];
#pragma unroll
                for (int q = 0; q < NM; ++q) h[q] = fmaf(w, dm[q][qy * IL_SW + px + k], h[q]);
            }
#pragma unroll
            for (int q = 0; q < NM; ++q) hm[q * (IL_SH * IL_TW) + i] = h[q];
        }
        __syncthreads();
    }
    // vertical + the pixel term + store: thread = pixel column px, pixel rows py and py + IL_TH / 2
    const int px = tid & (IL_TW - 1);
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int py = (tid / IL_TW) + half * (IL_TH / 2);
        const int y = cy0 + py, x = cx0 + px;                         // view coordinates
        if (y + g.crop >= g.H || x + g.crop >= g.W) continue;         // past the image (ragged last tiles)
        const bool inside = y >= 0 && y < g.Hc && x >= 0 && x < g.Wc;
        const int64_t off = base + (int64_t)(y + g.crop) * g.W + (x + g.crop);
        float ga = 0.f, gb = 0.f;
        if (inside) {
            float va, vb;
            if (g.with_ssim) {
                float tq[NM];
#pragma unroll
                for (int q = 0; q < NM; ++q) tq[q] = 0.f;
#pragma unroll
                for (int k = 0; k < IL_WIN; ++k) {
                    const float w = win.w[k];
#pragma unroll
                    for (int q = 0; q < NM; ++q) tq[q] = fmaf(w, hm[q * (IL_SH * IL_TW) + (py + k) * IL_TW + px], tq[q]);
                }
                va = sa[(py + IL_APRON) * IL_BW + px + IL_APRON];
                vb = sb[(py + IL_APRON) * IL_BW + px + IL_APRON];
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
    ImageLossGeom g;
    if (N <= 0) return SISR_E_BADARG;
    if (!image_loss_geom(C, H, W, crop, luma, with_ssim, g)) return (C != 1 && C != 3) ? SISR_E_UNSUPPORTED : SISR_E_BADARG;
    const int64_t floats = 2 * (int64_t)N * g.planes * g.tiles_y * g.tiles_x;
    return floats > INT32_MAX ? SISR_E_TOOBIG : (int)floats;
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
    ImageLossGeom g;
    image_loss_geom(C, H, W, crop, luma, with_ssim, g);
    const double L = (double)data_range;
    const int per_image = g.planes * g.tiles_y * g.tiles_x;
    hipStream_t st = sisr_stream(stream);
    hipLaunchKernelGGL(image_loss_tile_kernel, dim3((unsigned)(ws / 2)), dim3(SISR_BLOCK), 0, st, a, b, g, image_loss_window(),
                       (float)(0.01 * L * 0.01 * L), (float)(0.03 * L * 0.03 * L), (int)pix_kind, eps * eps, work);
    SISR_CHECK_LAUNCH();
    hipLaunchKernelGGL(image_loss_finish_kernel, dim3((unsigned)N), dim3(SISR_BLOCK), 0, st, (const float*)work, per_image,
                       with_ssim, (double)g.planes * g.Hv * g.Wv, (double)g.planes * g.Hc * g.Wc, (double)w_ssim, (double)w_pix,
                       loss, ssim, pix);
    SISR_CHECK_LAUNCH();
    return 0;
}

extern "C" int sisr_image_loss_bwd(const float* a, const float* b, const float* gup, int32_t N, int32_t C, int32_t H, int32_t W,
                                   int32_t crop, int32_t luma, float data_range, float w_ssim, float w_pix, int32_t pix_kind,
                                   float eps, float* da, float* db, void* stream) {
    const int with_ssim = w_ssim != 0.f ? 1 : 0;
    ImageLossGeom g;
    if (N <= 0) return SISR_E_BADARG;
    if (!image_loss_geom(C, H, W, crop, luma, with_ssim, g)) return (C != 1 && C != 3) ? SISR_E_UNSUPPORTED : SISR_E_BADARG;
    if (!a || !b || !gup || (!da && !db) || !image_loss_scalars_ok(data_range, pix_kind, eps)) return SISR_E_BADARG;
    const int64_t wgs = (int64_t)N * g.planes * g.btiles_y * g.btiles_x;
    if (wgs > INT32_MAX) return SISR_E_TOOBIG;
    const double L = (double)data_range;
    const float c1 = (float)(0.01 * L * 0.01 * L), c2 = (float)(0.03 * L * 0.03 * L);
    const float ks = with_ssim ? (float)(-(double)w_ssim / ((double)g.planes * g.Hv * g.Wv)) : 0.f;
    const float kp = (float)((double)w_pix / ((double)g.planes * g.Hc * g.Wc));
    const int kind = w_pix != 0.f ? (int)pix_kind : IL_PIX_NONE;
    const ImageLossWindow win = image_loss_window();
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
