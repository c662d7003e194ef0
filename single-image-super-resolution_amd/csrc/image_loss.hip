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
// Backward: one launch of the tile scheme of sisr_ssim_bwd.h (gather form, nothing saved by the forward but the inputs: a 16 x 32
// pixel tile of the WHOLE image per workgroup, the window moments recomputed in LDS, the derivative maps of the SSIM map filtered
// by the transposed window): the window gradient times -w_ssim g[n] / (C' Hv Wv), plus the pixel term's gradient.  Without the
// SSIM term (apron 0) nothing goes through LDS.  LDS: 62,688 B per workgroup.

// the forward under the compiler's default contraction, then contraction off to the end of this file (the include-order rule is
// written down in this header)
#include "sisr_ssim_bwd.h"

#define IL_PIX_NONE (-1)                      // internal: w_pix == 0, the pixel term contributes no gradient

// rho'(d); L1: 0 at d == 0 (torch's sign)
__device__ __forceinline__ float il_rho_grad(float d, int kind, float eps2) {
    if (kind == SISR_PIX_L1) return d > 0.f ? 1.f : d < 0.f ? -1.f : 0.f;
    if (kind == SISR_PIX_CHARBONNIER) return d / sqrtf(fmaf(d, d, eps2));
    return kind == SISR_PIX_MSE ? 2.f * d : 0.f;
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

// the workgroups of ssim_bwd_tile.  WA / WB: da / db wanted.  ks = -w_ssim / (C' Hv Wv), kp = w_pix / (C' H' W'): the factors of
// the two terms in front of the upstream gradient g[n]
template <bool WA, bool WB>
__global__ void __launch_bounds__(SISR_BLOCK) image_loss_bwd_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                    const float* __restrict__ gup, SsimGeom g,
                                                                    SsimWindow win, float c1, float c2, int pix_kind,
                                                                    float eps2, float ks, float kp, float* __restrict__ da,
                                                                    float* __restrict__ db) {
    __shared__ SsimBwdLds lds;
    const SsimBwdTile t = ssim_bwd_tile(g);
    const float gn = gup[t.n];
    const float ksn = gn * ks, kpn = gn * kp;
    if (g.apron) ssim_bwd_filter_maps<WA, WB, SSIM_MAP_LCS>(a, b, g, win, c1, c2, t, lds);
    ssim_bwd_pixels<WA, WB>(g, t, da, db, [&](int py, int px, int, int, int64_t off, float& ga, float& gb) {
        float va, vb;
        if (g.apron) {
            ssim_bwd_window_grad<WA, WB>(win, lds, py, px, va, vb, ga, gb);
            if (WA) ga = ksn * ga;
            if (WB) gb = ksn * gb;
        } else {
            va = ssim_view_load(a, off, t.plane_elems, g.luma);
            vb = ssim_view_load(b, off, t.plane_elems, g.luma);
        }
        const float dp = kpn * il_rho_grad(va - vb, pix_kind, eps2);
        ga += dp;
        gb -= dp;
    });
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
    float c1, c2;
    ssim_constants((double)data_range, c1, c2);
    const float ks = with_ssim ? (float)(-(double)w_ssim / ((double)g.planes * g.Hv * g.Wv)) : 0.f;
    const float kp = (float)((double)w_pix / ((double)g.planes * g.Hc * g.Wc));
    const int kind = w_pix != 0.f ? (int)pix_kind : IL_PIX_NONE;
    const SsimWindow win = ssim_window();
    hipStream_t st = sisr_stream(stream);
    ssim_bwd_dispatch(da, db, [&](auto wa, auto wb) {
        hipLaunchKernelGGL((image_loss_bwd_kernel<decltype(wa)::value, decltype(wb)::value>), dim3((unsigned)wgs), dim3(SISR_BLOCK), 0,
                           st, a, b, gup, g, win, c1, c2, kind, eps * eps, ks, kp, da, db);
    });
    SISR_CHECK_LAUNCH();
    return 0;
}
