// metrics.hip -- per-image PSNR and SSIM of two fp32 NCHW image batches, entirely on the device: the validation numbers of a
// super-resolution trainer without a device -> host copy in the middle of the loop (nothing here synchronises with the host, so
// the two launches can sit inside a captured step).
//
// The view (`crop`, `luma`), the SSIM definition and the tile scheme are sisr_ssim.h's: this file launches its tile kernel with the
// squared difference as the pixel term (the instantiation the image loss uses for 'mse' with its SSIM term) and finishes with
//   PSNR[n] = 10 log10(data_range^2 / mean_{C',H',W'} (a - b)^2)                                (+inf when the images are equal)
#include "sisr_ssim.h"

// one workgroup per image: the image's partials folded in double (ssim_fold_image)
__global__ void __launch_bounds__(SISR_BLOCK) metrics_finish_kernel(const float* __restrict__ part, int per_image, double n_ssim,
                                                                    double n_pix, double range2, float* __restrict__ psnr,
                                                                    float* __restrict__ ssim) {
    double s[2];
    ssim_fold_image(part, per_image, s);
    if (threadIdx.x == 0) {
        if (ssim) ssim[blockIdx.x] = (float)(s[0] / n_ssim);
        if (psnr) {
            const double mse = s[1] / n_pix;
            psnr[blockIdx.x] = mse > 0.0 ? (float)(10.0 * log10(range2 / mse)) : INFINITY;
        }
    }
}

extern "C" int sisr_image_metrics_ws_floats(int32_t N, int32_t C, int32_t H, int32_t W, int32_t crop, int32_t luma) {
    return ssim_ws_floats(N, C, H, W, crop, luma, SSIM_APRON);
}

extern "C" int sisr_image_metrics(const float* a, const float* b, int32_t N, int32_t C, int32_t H, int32_t W, int32_t crop,
                                  int32_t luma, float data_range, float* work, float* psnr, float* ssim, void* stream) {
    const int ws = sisr_image_metrics_ws_floats(N, C, H, W, crop, luma);
    if (ws < 0) return ws;
    if (!a || !b || !work || (!psnr && !ssim) || !(data_range > 0.f)) return SISR_E_BADARG;
    SsimGeom g;
    ssim_geom(C, H, W, crop, luma, SSIM_APRON, g);
    const double L = (double)data_range;
    hipStream_t st = sisr_stream(stream);
    const int e = ssim_launch_tiles<SISR_PIX_MSE, SSIM_APRON>(ws, st, a, b, g, L, ssim != nullptr ? 1 : 0, 0.f, work);
    if (e) return e;
    hipLaunchKernelGGL(metrics_finish_kernel, dim3((unsigned)N), dim3(SISR_BLOCK), 0, st, (const float*)work,
                       g.planes * g.tiles_y * g.tiles_x, (double)g.planes * g.Hv * g.Wv, (double)g.planes * g.Hc * g.Wc, L * L, psnr,
                       ssim);
    SISR_CHECK_LAUNCH();
    return 0;
}
