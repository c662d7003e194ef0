// metrics.hip -- per-image PSNR and SSIM of two fp32 NCHW image batches, entirely on the device: the validation numbers of a
// super-resolution trainer without a device -> host copy in the middle of the loop (nothing here synchronises with the host, so
// the two launches can sit inside a captured step).
//
// Input view (applied while staging, never materialised): `crop` pixels stripped from each side (H' = H - 2 crop, W' = W - 2 crop)
// and, for C == 3 with `luma`, the BT.601 full-range plane Y = 0.299 R + 0.587 G + 0.114 B in place of the three planes (C' = 1).
//   PSNR[n] = 10 log10(data_range^2 / mean_{C',H',W'} (a - b)^2)                                (+inf when the images are equal)
//   SSIM[n] = mean over C' and the (H' - 10) x (W' - 10) "valid" window positions of
//             ((2 mu_a mu_b + C1)(2 s_ab + C2)) / ((mu_a^2 + mu_b^2 + C1)(s_a^2 + s_b^2 + C2)),   C1 = (0.01 L)^2, C2 = (0.03 L)^2,
//             moments under the separable 11 x 11 Gaussian window (sigma 1.5, weights summing to 1: no sample-variance correction)
//
// One workgroup owns a MT_TH x MT_TW tile of window positions of one (image, plane): it stages the (MT_TH + 10) x (MT_TW + 10)
// pixels under those windows of a and b into LDS once, filters the five moments (a, b, a^2, b^2, ab) horizontally into LDS and
// vertically from it, forms the SSIM values in registers and leaves ONE partial (sum of SSIM values, sum of squared differences)
// in the workspace.  The squared differences ride on the staging pass: the tile grid partitions the cropped image as well when
// the tiles of the last row / column also take the 10 pixels behind them, so every pixel is counted by exactly one workgroup.
// metrics_finish_kernel adds an image's partials in a fixed order in double.  No atomics: the results are the same bits every call.
// LDS: 2 x 26 x 42 staged pixels + 5 x 26 x 32 row-filtered moments + 8 floats = 25.4 KB per workgroup.
#include "sisr_dev.h"

#include <cmath>

#define MT_WIN 11
#define MT_APRON (MT_WIN - 1)
#define MT_TH 16
#define MT_TW 32
#define MT_SH (MT_TH + MT_APRON)
#define MT_SW (MT_TW + MT_APRON)
static_assert(MT_TH * MT_TW == 2 * SISR_BLOCK, "the vertical pass gives every thread two window positions");

struct MetricsWindow { float w[MT_WIN]; };

struct MetricsGeom {
    int C, H, W, crop, luma;
    int Hc, Wc;                  // cropped image
    int Hv, Wv;                  // window positions
    int planes;                  // C'
    int tiles_y, tiles_x;
};

// false: the shapes are outside what the kernels take
static bool metrics_geom(int C, int H, int W, int crop, int luma, MetricsGeom& g) {
    if ((C != 1 && C != 3) || crop < 0 || H <= 0 || W <= 0) return false;
    g.C = C; g.H = H; g.W = W; g.crop = crop;
    g.luma = (luma != 0 && C == 3) ? 1 : 0;
    const int64_t hc = (int64_t)H - 2 * (int64_t)crop, wc = (int64_t)W - 2 * (int64_t)crop;
    if (hc < MT_WIN || wc < MT_WIN) return false;
    g.Hc = (int)hc; g.Wc = (int)wc;
    g.Hv = g.Hc - MT_APRON; g.Wv = g.Wc - MT_APRON;
    g.planes = g.luma ? 1 : C;
    g.tiles_y = (g.Hv + MT_TH - 1) / MT_TH;
    g.tiles_x = (g.Wv + MT_TW - 1) / MT_TW;
    return true;
}

// workgroup = (image n, plane, tile row, tile column), flat in that order; part[workgroup][2] = (sum of SSIM values, sum of
// squared differences)
__global__ void __launch_bounds__(SISR_BLOCK) metrics_tile_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                  MetricsGeom g, MetricsWindow win, float c1, float c2,
                                                                  int do_ssim, float* __restrict__ part) {
    __shared__ float sa[MT_SH * MT_SW], sb[MT_SH * MT_SW];
    __shared__ float hm[5][MT_SH * MT_TW];
    const int tid = threadIdx.x;
    const int tiles = g.tiles_y * g.tiles_x, per_image = g.planes * tiles;
    const int n = blockIdx.x / per_image, r = blockIdx.x - n * per_image;
    const int plane = r / tiles, t = r - plane * tiles;
    const int ty = t / g.tiles_x, tx = t - ty * g.tiles_x;
    const int y0 = ty * MT_TH, x0 = tx * MT_TW;                       // tile origin in the cropped image
    // pixels this workgroup counts for the PSNR: its MT_TH x MT_TW block, and everything behind it in the last row / column
    const int own_h = ty == g.tiles_y - 1 ? MT_SH : MT_TH, own_w = tx == g.tiles_x - 1 ? MT_SW : MT_TW;
    const int64_t plane_elems = (int64_t)g.H * g.W;
    const int64_t base = ((int64_t)n * g.C + (g.luma ? 0 : plane)) * plane_elems;
    float ss_sq[2] = {0.f, 0.f};          // sum of SSIM values, sum of squared differences
    float &ss = ss_sq[0], &sq = ss_sq[1];
    for (int i = tid; i < MT_SH * MT_SW; i += SISR_BLOCK) {
        const int ly = i / MT_SW, lx = i - ly * MT_SW;
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
            if (ly < own_h && lx < own_w) sq += (va - vb) * (va - vb);
        }
        sa[i] = va;
        sb[i] = vb;
    }
    if (do_ssim) {
        __syncthreads();
        // horizontal pass: every staged row, MT_TW window columns (lanes on consecutive columns: conflict-free LDS reads)
        for (int i = tid; i < MT_SH * MT_TW; i += SISR_BLOCK) {
            const int ly = i / MT_TW, ox = i - ly * MT_TW;
            const float* pa = sa + ly * MT_SW + ox;
            const float* pb = sb + ly * MT_SW + ox;
            float ma = 0.f, mb = 0.f, maa = 0.f, mbb = 0.f, mab = 0.f;
#pragma unroll
            for (int k = 0; k < MT_WIN; ++k) {
                const float w = win.w[k], u = pa[k], v = pb[k];
                const float wu = w * u, wv = w * v;
                ma += wu; mb += wv;
                maa = fmaf(wu, u, maa); mbb = fmaf(wv, v, mbb); mab = fmaf(wu, v, mab);
            }
            hm[0][i] = ma; hm[1][i] = mb; hm[2][i] = maa; hm[3][i] = mbb; hm[4][i] = mab;
        }
        __syncthreads();
        // vertical pass + SSIM map: thread = window column ox, window rows oy and oy + MT_TH / 2
        const int ox = tid & (MT_TW - 1);
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const int oy = (tid / MT_TW) + half * (MT_TH / 2);
            float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < MT_WIN; ++k) {
                const float w = win.w[k];
#pragma unroll
                for (int q = 0; q < 5; ++q) m[q] = fmaf(w, hm[q][(oy + k) * MT_TW + ox], m[q]);
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

// one workgroup per image: the image's partials added in a fixed order in double (fold_partials_double)
__global__ void __launch_bounds__(SISR_BLOCK) metrics_finish_kernel(const float* __restrict__ part, int per_image, double n_ssim,
                                                                    double n_pix, double range2, float* __restrict__ psnr,
                                                                    float* __restrict__ ssim) {
    const float* p = part + 2 * (int64_t)blockIdx.x * per_image;
    double s[2];
    fold_partials_double(per_image, s, [&](int64_t i, double* acc) { acc[0] += (double)p[2 * i]; acc[1] += (double)p[2 * i + 1]; });
    if (threadIdx.x == 0) {
        if (ssim) ssim[blockIdx.x] = (float)(s[0] / n_ssim);
        if (psnr) {
            const double mse = s[1] / n_pix;
            psnr[blockIdx.x] = mse > 0.0 ? (float)(10.0 * log10(range2 / mse)) : INFINITY;
        }
    }
}

extern "C" int sisr_image_metrics_ws_floats(int32_t N, int32_t C, int32_t H, int32_t W, int32_t crop, int32_t luma) {
    MetricsGeom g;
    if (N <= 0) return SISR_E_BADARG;
    if (!metrics_geom(C, H, W, crop, luma, g)) return (C != 1 && C != 3) ? SISR_E_UNSUPPORTED : SISR_E_BADARG;
    const int64_t floats = 2 * (int64_t)N * g.planes * g.tiles_y * g.tiles_x;
    return floats > INT32_MAX ? SISR_E_TOOBIG : (int)floats;
}

extern "C" int sisr_image_metrics(const float* a, const float* b, int32_t N, int32_t C, int32_t H, int32_t W, int32_t crop,
                                  int32_t luma, float data_range, float* work, float* psnr, float* ssim, void* stream) {
    const int ws = sisr_image_metrics_ws_floats(N, C, H, W, crop, luma);
    if (ws < 0) return ws;
    if (!a || !b || !work || (!psnr && !ssim) || !(data_range > 0.f)) return SISR_E_BADARG;
    MetricsGeom g;
    metrics_geom(C, H, W, crop, luma, g);
    // the 11-tap Gaussian, sigma 1.5, normalised in double
    MetricsWindow win;
    double wd[MT_WIN], sum = 0.0;
    for (int k = 0; k < MT_WIN; ++k) {
        const double d = (double)(k - MT_WIN / 2);
        wd[k] = exp(-d * d / (2.0 * 1.5 * 1.5));
        sum += wd[k];
    }
    for (int k = 0; k < MT_WIN; ++k) win.w[k] = (float)(wd[k] / sum);
    const double L = (double)data_range;
    const int per_image = g.planes * g.tiles_y * g.tiles_x;
    hipStream_t st = sisr_stream(stream);
    hipLaunchKernelGGL(metrics_tile_kernel, dim3((unsigned)(ws / 2)), dim3(SISR_BLOCK), 0, st, a, b, g, win,
                       (float)(0.01 * L * 0.01 * L), (float)(0.03 * L * 0.03 * L), ssim != nullptr ? 1 : 0, work);
    SISR_CHECK_LAUNCH();
    hipLaunchKernelGGL(metrics_finish_kernel, dim3((unsigned)N), dim3(SISR_BLOCK), 0, st, (const float*)work, per_image,
                       (double)g.planes * g.Hv * g.Wv, (double)g.planes * g.Hc * g.Wc, L * L, psnr, ssim);
    SISR_CHECK_LAUNCH();
    return 0;
}
