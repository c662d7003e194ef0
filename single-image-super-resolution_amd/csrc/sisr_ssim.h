// sisr_ssim.h -- the forward SSIM tile scheme, once, for its two callers: the metric (metrics.hip) and the image loss
// (image_loss.hip); the geometry, the window, the constants and the workgroup decode also serve MS-SSIM (ms_ssim.hip) and the
// backward scheme (sisr_ssim_bwd.h).  Per image of two fp32 NCHW batches, on a view applied while staging and never materialised (`crop` pixels
// stripped from each side: H' = H - 2 crop, W' = W - 2 crop; for C == 3 with `luma` the BT.601 full-range plane
// Y = 0.299 R + 0.587 G + 0.114 B in place of the three planes, C' = 1):
//   SSIM[n] = mean over C' and the (H' - 10) x (W' - 10) "valid" window positions of
//             ((2 mu_a mu_b + C1)(2 s_ab + C2)) / ((mu_a^2 + mu_b^2 + C1)(s_a^2 + s_b^2 + C2)),   C1 = (0.01 L)^2, C2 = (0.03 L)^2,
//             moments under the separable 11 x 11 Gaussian window (sigma 1.5, weights summing to 1: no sample-variance correction)
//   pixel term[n] = mean_{C',H',W'} rho(a - b),   rho(d) = d^2 (the metric's PSNR, the loss's 'mse') / |d| / sqrt(d^2 + eps^2)
//
// One workgroup owns a SSIM_TH x SSIM_TW tile of window positions of one (image, plane): it stages the (SSIM_TH + 10) x
// (SSIM_TW + 10) pixels under those windows of a and b into LDS once, filters the five moments (a, b, a^2, b^2, ab) horizontally
// into LDS and vertically from it, forms the SSIM values in registers and leaves ONE partial (sum of SSIM values, sum of rho) in
// the workspace.  The pixel term rides on the staging pass: the tile grid partitions the view as well when the tiles of the last
// row / column also take the 10 pixels behind them, so every pixel is counted by exactly one workgroup.  With apron 0 (a loss
// without its SSIM term) the grid partitions the view itself into SSIM_TH x SSIM_TW pixel tiles and nothing goes through LDS.
// ssim_fold_image adds an image's partials in a fixed order in double.  No atomics: the results are the same bits every call.
// LDS: 2 x 26 x 42 staged pixels + 5 x 26 x 32 row-filtered moments + 8 floats = 25.4 KB per workgroup.
//
// Rounding: this header is compiled under the compiler's default contraction, and every caller gets the same instructions from it:
// the SSIM of the loss is the metric's bit for bit.  The backward scheme (sisr_ssim_bwd.h) includes this header FIRST and only
// then switches contraction off for itself and for the rest of the including file; it keeps a row pass of its own under that
// pragma, because its instantiations must round every product as written for da to be the same bits whether or not db is asked for.
#pragma once
#include "sisr_dev.h"

#include <cmath>

#define SSIM_WIN 11
#define SSIM_APRON (SSIM_WIN - 1)
#define SSIM_TH 16
#define SSIM_TW 32
#define SSIM_SH (SSIM_TH + SSIM_APRON)        // forward: staged pixels; the loss backward: window positions that touch a pixel tile
#define SSIM_SW (SSIM_TW + SSIM_APRON)
static_assert(SSIM_TH * SSIM_TW == 2 * SISR_BLOCK, "the last pass gives every thread two pixels / window positions");

struct SsimWindow { float w[SSIM_WIN]; };

struct SsimGeom {
    int C, H, W, crop, luma, apron;
    int Hc, Wc;                  // the view
    int Hv, Wv;                  // window positions (apron 0: the view's pixels)
    int planes;                  // C'
    int tiles_y, tiles_x;        // forward grid: over Hv x Wv
    int btiles_y, btiles_x;      // the loss backward's grid: over the whole image's pixels
};

// apron: SSIM_APRON, or 0 for a pixel term alone (any view of at least one pixel).  false: the shapes are outside what the
// kernels take
static bool ssim_geom(int C, int H, int W, int crop, int luma, int apron, SsimGeom& g) {
    if ((C != 1 && C != 3) || crop < 0 || H <= 0 || W <= 0) return false;
    g.C = C; g.H = H; g.W = W; g.crop = crop; g.apron = apron;
    g.luma = (luma != 0 && C == 3) ? 1 : 0;
    const int64_t hc = (int64_t)H - 2 * (int64_t)crop, wc = (int64_t)W - 2 * (int64_t)crop;
    if (hc <= apron || wc <= apron) return false;
    g.Hc = (int)hc; g.Wc = (int)wc;
    g.Hv = g.Hc - apron; g.Wv = g.Wc - apron;
    g.planes = g.luma ? 1 : C;
    g.tiles_y = (g.Hv + SSIM_TH - 1) / SSIM_TH;
    g.tiles_x = (g.Wv + SSIM_TW - 1) / SSIM_TW;
    g.btiles_y = (H + SSIM_TH - 1) / SSIM_TH;
    g.btiles_x = (W + SSIM_TW - 1) / SSIM_TW;
    return true;
}

// the workspace of the forward: one (sum of SSIM values, sum of rho) pair per workgroup; < 0: a status code
static int ssim_ws_floats(int N, int C, int H, int W, int crop, int luma, int apron) {
    SsimGeom g;
    if (N <= 0) return SISR_E_BADARG;
    if (!ssim_geom(C, H, W, crop, luma, apron, g)) return (C != 1 && C != 3) ? SISR_E_UNSUPPORTED : SISR_E_BADARG;
    const int64_t floats = 2 * (int64_t)N * g.planes * g.tiles_y * g.tiles_x;
    return floats > INT32_MAX ? SISR_E_TOOBIG : (int)floats;
}

// the 11-tap Gaussian, sigma 1.5, normalised in double
static SsimWindow ssim_window() {
    SsimWindow win;
    double wd[SSIM_WIN], sum = 0.0;
    for (int k = 0; k < SSIM_WIN; ++k) {
        const double d = (double)(k - SSIM_WIN / 2);
        wd[k] = exp(-d * d / (2.0 * 1.5 * 1.5));
        sum += wd[k];
    }
    for (int k = 0; k < SSIM_WIN; ++k) win.w[k] = (float)(wd[k] / sum);
    return win;
}

// a workgroup of a flat grid over (image n, plane, tile row, tile column), in that order; base: the first element of the plane
// (of plane 0 under luma)
struct SsimTile {
    int n, plane, ty, tx;
    int64_t plane_elems, base;
};

__device__ __forceinline__ SsimTile ssim_tile(const SsimGeom& g, int tiles_y, int tiles_x) {
    SsimTile t;
    const int tiles = tiles_y * tiles_x, per_image = g.planes * tiles;
    t.n = blockIdx.x / per_image;
    const int r = blockIdx.x - t.n * per_image;
    t.plane = r / tiles;
    const int q = r - t.plane * tiles;
    t.ty = q / tiles_x;
    t.tx = q - t.ty * tiles_x;
    t.plane_elems = (int64_t)g.H * g.W;
    t.base = ((int64_t)t.n * g.C + (g.luma ? 0 : t.plane)) * t.plane_elems;
    return t;
}

// C1 = (0.01 L)^2, C2 = (0.03 L)^2 as the kernels take them
static void ssim_constants(double L, float& c1, float& c2) {
    c1 = (float)(0.01 * L * 0.01 * L);
    c2 = (float)(0.03 * L * 0.03 * L);
}

// workgroup = (image n, plane, tile row, tile column), flat in that order; part[workgroup][2] = (sum of SSIM values, sum of rho).
// PIX: the pixel term, a SISR_PIX_* (the squared difference is spelled in place: what the backend contracts there is the
// metric's arithmetic).  APRON: SSIM_APRON, or 0 (do_ssim is 0 then)
template <int PIX, int APRON>
__global__ void __launch_bounds__(SISR_BLOCK) ssim_tile_kernel(const float* __restrict__ a, const float* __restrict__ b, SsimGeom g,
                                                               SsimWindow win, float c1, float c2, int do_ssim, float eps2,
                                                               float* __restrict__ part) {
    constexpr int SH = SSIM_TH + APRON, SW = SSIM_TW + APRON;
    __shared__ float sa[SH * SW], sb[SH * SW];
    __shared__ float hm[5][SH * SSIM_TW];
    const int tid = threadIdx.x;
    const int tiles = g.tiles_y * g.tiles_x, per_image = g.planes * tiles;
    const int n = blockIdx.x / per_image, r = blockIdx.x - n * per_image;
    const int plane = r / tiles, t = r - plane * tiles;
    const int ty = t / g.tiles_x, tx = t - ty * g.tiles_x;
    const int y0 = ty * SSIM_TH, x0 = tx * SSIM_TW;                   // tile origin in the view
    // pixels this workgroup counts for the pixel term: its SSIM_TH x SSIM_TW block, and everything behind it in the last row /
    // column
    const int own_h = ty == g.tiles_y - 1 ? SH : SSIM_TH, own_w = tx == g.tiles_x - 1 ? SW : SSIM_TW;
    const int64_t plane_elems = (int64_t)g.H * g.W;
    const int64_t base = ((int64_t)n * g.C + (g.luma ? 0 : plane)) * plane_elems;
    float ss_sq[2] = {0.f, 0.f};          // sum of SSIM values, sum of rho (the metric: of squared differences)
    float &ss = ss_sq[0], &sq = ss_sq[1];
    for (int i = tid; i < SH * SW; i += SISR_BLOCK) {
        const int ly = i / SW, lx = i - ly * SW;
        const int y = y0 + ly, x = x0 + lx;
        float va = 0.f, vb = 0.f;
        if (y < g.Hc && x < g.Wc) {
            const int64_t off = base + (int64_t)(y + g.crop) * g.W + (x + g.crop);
            if (g.luma) {
                va = 0.299f * a[off] + 0.587f * a[off + plane_elems] + 0.114f * a[off + 2 * plane_elems];
                vb = 0.299f * b[off] + 0.587f * b[off + plane_elems] + 0.114f * b[off + 2 * plane_elems];
            } else {
                va = a[off];
                vb = b[off];
            }
            if (ly < own_h && lx < own_w) {
                if constexpr (PIX == SISR_PIX_MSE) sq += (va - vb) * (va - vb);
                else sq += PIX == SISR_PIX_L1 ? fabsf(va - vb) : sqrtf(fmaf(va - vb, va - vb, eps2));
            }
        }
        if constexpr (APRON != 0) {
            sa[i] = va;
            sb[i] = vb;
        }
    }
    if constexpr (APRON != 0) if (do_ssim) {
        __syncthreads();
        // horizontal pass: every staged row, SSIM_TW window columns (lanes on consecutive columns: conflict-free LDS reads)
        for (int i = tid; i < SH * SSIM_TW; i += SISR_BLOCK) {
            const int ly = i / SSIM_TW, ox = i - ly * SSIM_TW;
            const float* pa = sa + ly * SW + ox;
            const float* pb = sb + ly * SW + ox;
            float ma = 0.f, mb = 0.f, maa = 0.f, mbb = 0.f, mab = 0.f;
#pragma unroll
            for (int k = 0; k < SSIM_WIN; ++k) {
                const float w = win.w[k], u = pa[k], v = pb[k];
                const float wu = w * u, wv = w * v;
                ma += wu; mb += wv;
                maa = fmaf(wu, u, maa); mbb = fmaf(wv, v, mbb); mab = fmaf(wu, v, mab);
            }
            hm[0][i] = ma; hm[1][i] = mb; hm[2][i] = maa; hm[3][i] = mbb; hm[4][i] = mab;
        }
        __syncthreads();
        // vertical pass + SSIM map: thread = window column ox, window rows oy and oy + SSIM_TH / 2
        const int ox = tid & (SSIM_TW - 1);
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const int oy = (tid / SSIM_TW) + half * (SSIM_TH / 2);
            float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < SSIM_WIN; ++k) {
                const float w = win.w[k];
#pragma unroll
                for (int q = 0; q < 5; ++q) m[q] = fmaf(w, hm[q][(oy + k) * SSIM_TW + ox], m[q]);
            }
            if (y0 + oy < g.Hv && x0 + ox < g.Wv) {
                const float mu_aa = m[0] * m[0], mu_bb = m[1] * m[1], mu_ab = m[0] * m[1];
                const float var_a = m[2] - mu_aa, var_b = m[3] - mu_bb, cov = m[4] - mu_ab;
                ss += ((2.f * mu_ab + c1) * (2.f * cov + c2)) / ((mu_aa + mu_bb + c1) * (var_a + var_b + c2));
            }
        }
    }
    block_partial_sum(ss_sq);
    if (tid == 0) {
        part[2 * (int64_t)blockIdx.x] = ss;
        part[2 * (int64_t)blockIdx.x + 1] = sq;
    }
}

// a finish kernel's first half, one workgroup per image: the image's partials added in a fixed order in double
// (fold_partials_double) -> s = (sum of SSIM values, sum of rho), valid in all threads
__device__ __forceinline__ void ssim_fold_image(const float* __restrict__ part, int per_image, double (&s)[2]) {
    const float* p = part + 2 * (int64_t)blockIdx.x * per_image;
    fold_partials_double(per_image, s, [&](int64_t i, double* acc) { acc[0] += (double)p[2 * i]; acc[1] += (double)p[2 * i + 1]; });
}

// the forward launch: ws_floats / 2 workgroups, L = data_range -> 0 or the launch's error
template <int PIX, int APRON>
static int ssim_launch_tiles(int ws_floats, hipStream_t st, const float* a, const float* b, const SsimGeom& g, double L, int do_ssim,
                             float eps2, float* work) {
    float c1, c2;
    ssim_constants(L, c1, c2);
    hipLaunchKernelGGL((ssim_tile_kernel<PIX, APRON>), dim3((unsigned)(ws_floats / 2)), dim3(SISR_BLOCK), 0, st, a, b, g,
                       ssim_window(), c1, c2, do_ssim, eps2, work);
    SISR_CHECK_LAUNCH();
    return 0;
}
