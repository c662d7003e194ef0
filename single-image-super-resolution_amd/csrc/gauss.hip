// gauss.hip -- a large-support separable Gaussian filter with a mirrored border, forward and backward, and the unsharp mask built
// on it.  Tensors are fp32 [N][C][H][W], contiguous; a plane is one (n, c).
//   y[i][j] = sum_{a, b} t[a] t[b] x[m(i + a - R)][m(j + b - R)],   R = K / 2, K odd, 1 .. SISR_GAUSS_MAX_K,
//   m(p) = -p for p < 0, 2 (L - 1) - p for p >= L (torch's 'reflect', OpenCV's BORDER_REFLECT_101); it needs H > R and W > R.
// One kernel text, gauss_tile_kernel<MODE>: a workgroup owns a GS_TH x GS_TW tile of one plane, stages tile + 2R rows x tile + 2R
// columns into LDS once (the border resolved while staging), filters along the rows into LDS and along the columns out of it.  Lanes
// sit on consecutive columns in both passes (conflict-free LDS reads; the taps are broadcast reads).  The row pass gives a thread GS_P
// rows of one column, so a tap is read once for GS_P products; the column pass slides a window of GS_P taps down one column, so
// a staged value is read once for GS_P products.  No intermediate goes to HBM.
//   GS_FWD       mirrored staging, y = G x
//   GS_BWD       the exact transpose in gather form: dy is staged ZERO-extended, correlated with the flipped taps over the padded
//                coordinates [-R, L - 1 + R] of each axis (z), and folded: dx[j] = z[j] + z[-j] [1 <= j <= R] +
//                z[2 (L - 1) - j] [L - 1 - R <= j <= L - 2].  The two folded terms of a pixel are gathered from the same staged
//                tile (they read pixels within R of it).  Fixed order, no atomics: the same bits on every call.
//   GS_USM_MASK  GS_FWD whose epilogue leaves blur = G x in the workspace and the bytes mask = |x - blur| s > threshold
//   GS_USM_MIX   stages the MASK bytes (mirrored), soft = G mask, and the epilogue reads x and blur again:
//                sharp = clamp(x + weight (x - blur), lo, hi),  y = x + soft (sharp - x)
// LDS at K = 63: 96 x 126 staged + 96 x 64 row-filtered floats + 72 taps = 73,248 bytes, two workgroups per CU; at K = 51 60,048.
// Plain vector stores only; nothing is read back by the host.
#include "sisr_dev.h"

#include <cmath>

#define GS_TH 32
#define GS_TW 64
#define GS_P 4
#define GS_SU 8
static_assert(GS_TW == 64 && SISR_BLOCK == 256, "a wave's lanes are the tile's columns; four waves share the rows");
static_assert(GS_TW + SISR_GAUSS_MAX_K - 1 <= 128, "the staging pass covers a row with two loads per lane");
static_assert(SISR_GAUSS_MAX_K % 2 == 1, "odd sizes only");

enum { GS_FWD = 0, GS_BWD = 1, GS_USM_MASK = 2, GS_USM_MIX = 3 };

struct GaussArgs {
    const float* x;          // what is staged (GS_USM_MIX: the image itself, read in the epilogue)
    const uint8_t* m;        // GS_USM_MIX: the mask bytes that are staged
    const float* taps;       // [K]
    float* y;
    float* blur;             // GS_USM_MASK writes it, GS_USM_MIX reads it
    uint8_t* mask;           // GS_USM_MASK: the workspace's mask bytes
    uint8_t* mask_out;       // GS_USM_MASK: the caller's copy, or NULL
    int H, W, K, tiles_x, tiles_y;
    float weight, threshold, lo, hi, scale;
};

// rows of the two LDS arrays, floats of the padded tap array (GS_P - 1 zeros in front, GS_P behind, rounded up to four)
__host__ __device__ static inline int gs_rows(int K) { return (GS_TH + K - 1 + GS_P - 1) & ~(GS_P - 1); }
__host__ __device__ static inline int gs_tap_floats(int K) { return (K + 2 * GS_P - 1 + 3) & ~3; }
static inline int gs_lds_bytes(int K) { return (int)sizeof(float) * (gs_tap_floats(K) + gs_rows(K) * (GS_TW + K - 1 + GS_TW)); }

template <int MODE>
__global__ void __launch_bounds__(SISR_BLOCK) gauss_tile_kernel(GaussArgs a) {
    extern __shared__ float gs_lds[];
    constexpr bool BWD = MODE == GS_BWD;
    const int K = a.K, R = K >> 1, H = a.H, W = a.W;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tiles = a.tiles_x * a.tiles_y;
    const int plane = blockIdx.x / tiles, t = blockIdx.x - plane * tiles;
    const int ty = t / a.tiles_x, tx = t - ty * a.tiles_x;
    const int y0 = ty * GS_TH, x0 = tx * GS_TW;
    const int th = min(GS_TH, H - y0), tw = min(GS_TW, W - x0);
    const int SW = GS_TW + 2 * R;                        // pitch of the staged tile
    float* tp = gs_lds;                                  // tp[GS_P - 1 + k] = tap k of the pass (the backward's: flipped), zeros around
    float* in = tp + gs_tap_floats(K);                   // [gs_rows][SW]
    float* tmp = in + gs_rows(K) * SW;                   // [gs_rows][GS_TW]
    const size_t base = (size_t)plane * (size_t)H * (size_t)W;

    for (int i = tid; i < gs_tap_floats(K); i += SISR_BLOCK) {
        const int k = i - (GS_P - 1);
        tp[i] = (k >= 0 && k < K) ? a.taps[BWD ? K - 1 - k : k] : 0.f;
    }
    // ---- staging: th + 2R rows x tw + 2R columns (at most 126: two lanes' worth), a wave per row, GS_SU rows of a wave per trip so
    // that 2 GS_SU loads are in flight before the first LDS store waits for one
    const int sr = th + 2 * R, sc = tw + 2 * R;
    for (int rb = wave; rb < sr; rb += GS_SU * (SISR_BLOCK / 64)) {
        float v[GS_SU][2];
#pragma unroll
        for (int u = 0; u < GS_SU; ++u) {
            const int r = rb + u * (SISR_BLOCK / 64);
            int gy = y0 - R + r;
            bool row_in = r < sr;
            if (BWD) row_in = row_in && gy >= 0 && gy < H;
            else gy = gy < 0 ? -gy : (gy >= H ? 2 * (H - 1) - gy : gy);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int c = lane + 64 * h;
                int gx = x0 - R + c;
                bool col_in = c < sc;
                if (BWD) col_in = col_in && gx >= 0 && gx < W;
                else gx = gx < 0 ? -gx : (gx >= W ? 2 * (W - 1) - gx : gx);
                v[u][h] = 0.f;
                if (row_in && col_in) {
                    const size_t off = base + (size_t)gy * W + gx;
                    v[u][h] = MODE == GS_USM_MIX ? (float)a.m[off] : a.x[off];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < GS_SU; ++u) {
            const int r = rb + u * (SISR_BLOCK / 64);
#pragma unroll
            for (int h = 0; h < 2; ++h)
                if (r < sr && lane + 64 * h < sc) in[r * SW + lane + 64 * h] = v[u][h];
        }
    }
    __syncthreads();

    // ---- along the rows: tmp[r][c] = sum_k tap[k] in[r][c + k] for the rows the column pass reads.  Rows past the staged ones are
    // stored as zeros: the sliding window below reads them for the pixels past the tile's last row, which are not stored
    const int rows_rp = ((th + GS_P - 1) & ~(GS_P - 1)) + 2 * R;
    if (lane < tw) {
        for (int g = wave; g * GS_P < rows_rp; g += SISR_BLOCK / 64) {
            const int r0 = g * GS_P;
            const float* src = in + r0 * SW + lane;
            float acc[GS_P];
#pragma unroll
            for (int j = 0; j < GS_P; ++j) acc[j] = 0.f;
#pragma unroll 4
            for (int k = 0; k < K; ++k) {
                const float w = tp[GS_P - 1 + k];
#pragma unroll
                for (int j = 0; j < GS_P; ++j) acc[j] = fmaf(w, src[j * SW + k], acc[j]);
            }
            if (BWD) {
                // z of the folded coordinates p of column jx: sum_k t[k] dy[p + R - k].  The loops run over the image column q = p + R - k,
                // the same for every lane (a broadcast read of the staged value); the tap index k is the lane's own (consecutive words)
                const int jx = x0 + lane;
                if (x0 == 0 && R > 0) {
                    // p = -jx for jx in 1 .. R (only the first tile column has them): q = 0 .. R - 1, k = R - jx - q
                    const bool on = jx >= 1 && jx <= R;
                    for (int q = 0; q < R; ++q) {
                        const int k = R - jx - q;
                        const float t = tp[GS_P - 1 + (K - 1 - min(max(k, 0), K - 1))];
                        const bool use = on && k >= 0;                 // a skipped term's VALUE is replaced by 0 as well: no 0 x Inf
                        const float w = use ? t : 0.f;
#pragma unroll
                        for (int j = 0; j < GS_P; ++j) {
                            const float v = in[(r0 + j) * SW + q + R];
                            acc[j] = fmaf(w, use ? v : 0.f, acc[j]);
                        }
                    }
                }
                if (x0 + tw - 1 >= W - 1 - R && R > 0) {
                    // p = 2 (W - 1) - jx for jx in W - 1 - R .. W - 2: q = W - 1 - R .. W - 1 (staged: this tile reaches that zone),
                    // k = p + R - q >= R + 1
                    const bool on = jx >= W - 1 - R && jx <= W - 2;
                    for (int q = W - 1 - R; q <= W - 1; ++q) {
                        const int k = 2 * (W - 1) - jx + R - q;
                        const float t = tp[GS_P - 1 + (K - 1 - min(max(k, 0), K - 1))];
                        const bool use = on && k <= 2 * R;
                        const float w = use ? t : 0.f;
#pragma unroll
                        for (int j = 0; j < GS_P; ++j) {
                            const float v = in[(r0 + j) * SW + q - x0 + R];
                            acc[j] = fmaf(w, use ? v : 0.f, acc[j]);
                        }
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < GS_P; ++j)
                if (r0 + j < rows_rp) tmp[(r0 + j) * GS_TW + lane] = r0 + j < sr ? acc[j] : 0.f;
        }
    }
    __syncthreads();

    // ---- along the columns: out[r0 + j] = sum_k tap[k] tmp[r0 + j + k]; the value of row r0 + i meets taps i, i - 1, ... i - GS_P + 1
    if (lane < tw) {
        for (int g = wave; g * GS_P < th; g += SISR_BLOCK / 64) {
            const int r0 = g * GS_P;
            const float* src = tmp + r0 * GS_TW + lane;
            float acc[GS_P], w[GS_P];
#pragma unroll
            for (int j = 0; j < GS_P; ++j) {
                acc[j] = 0.f;
                w[j] = tp[GS_P - 1 - j];
            }
            // row r0 + i belongs to pixel j only for 0 <= i - j < K: true for every j in the middle steps; in the first and the last
            // GS_P - 1 steps the others take 0 in place of the value (their tap is a zero of the padded array, and 0 x Inf would
            // carry a non-finite value out of the filter's support)
            auto step = [&](int i, bool guarded) {
                const float v = src[i * GS_TW];
#pragma unroll
                for (int j = 0; j < GS_P; ++j) acc[j] = fmaf(w[j], !guarded || (i >= j && i - j < K) ? v : 0.f, acc[j]);
#pragma unroll
                for (int j = GS_P - 1; j > 0; --j) w[j] = w[j - 1];
                w[0] = tp[GS_P + i];
            };
#pragma unroll
            for (int i = 0; i < GS_P - 1; ++i) step(i, true);
#pragma unroll 4
            for (int i = GS_P - 1; i < K; ++i) step(i, false);
            for (int i = max(K, GS_P - 1); i < K + GS_P - 1; ++i) step(i, true);
            if (BWD && R > 0) {
                // the folded terms of the rows, as above: the loops run over the image row q, one read of its row-filtered value
                // for the GS_P pixels, each with the tap of its own k (a broadcast read)
                const int jy0 = y0 + r0;
                if (y0 == 0 && r0 <= R) {
                    for (int q = 0; q < R; ++q) {                      // p = -jy for jy in 1 .. R: k = R - jy - q
                        const float v = tmp[(q + R) * GS_TW + lane];
#pragma unroll
                        for (int j = 0; j < GS_P; ++j) {
                            const int jy = jy0 + j, k = R - jy - q;
                            const float t = tp[GS_P - 1 + (K - 1 - min(max(k, 0), K - 1))];
                            const bool use = jy >= 1 && jy <= R && k >= 0;
                            acc[j] = fmaf(use ? t : 0.f, use ? v : 0.f, acc[j]);
                        }
                    }
                }
                if (jy0 + GS_P - 1 >= H - 1 - R) {
                    for (int q = H - 1 - R; q <= H - 1; ++q) {         // p = 2 (H - 1) - jy for jy in H - 1 - R .. H - 2: k = p + R - q
                        const float v = tmp[(q - y0 + R) * GS_TW + lane];
#pragma unroll
                        for (int j = 0; j < GS_P; ++j) {
                            const int jy = jy0 + j, k = 2 * (H - 1) - jy + R - q;
                            const float t = tp[GS_P - 1 + (K - 1 - min(max(k, 0), K - 1))];
                            const bool use = jy >= H - 1 - R && jy <= H - 2 && k <= 2 * R;
                            acc[j] = fmaf(use ? t : 0.f, use ? v : 0.f, acc[j]);
                        }
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < GS_P; ++j) {
                const int r = r0 + j;
                if (r >= th) continue;
                const size_t off = base + (size_t)(y0 + r) * W + (x0 + lane);
                if (MODE == GS_FWD || MODE == GS_BWD) {
                    a.y[off] = acc[j];
                } else if (MODE == GS_USM_MASK) {
                    const float res = in[(r + R) * SW + lane + R] - acc[j];
                    const uint8_t mk = fabsf(res) * a.scale > a.threshold ? 1 : 0;
                    a.blur[off] = acc[j];
                    a.mask[off] = mk;
                    if (a.mask_out) a.mask_out[off] = mk;
                } else {
                    const float xv = a.x[off];
                    const float res = xv - a.blur[off];
                    const float sharp = fminf(fmaxf(fmaf(a.weight, res, xv), a.lo), a.hi);
                    a.y[off] = fmaf(acc[j], sharp - xv, xv);
                }
            }
        }
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
extern "C" int sisr_gauss_taps_host(int32_t K, float sigma, float* taps_host) {
    if (!taps_host || K < 1 || K > SISR_GAUSS_MAX_K || K % 2 == 0 || sigma != sigma || std::isinf(sigma)) return SISR_E_BADARG;
    const double s = sigma > 0.f ? (double)sigma : 0.3 * ((K - 1) * 0.5 - 1.0) + 0.8;
    double t[SISR_GAUSS_MAX_K], sum = 0.0;
    for (int i = 0; i < K; ++i) {
        const double d = (double)i - (K - 1) * 0.5;
        t[i] = exp(-d * d / (2.0 * s * s));
        sum += t[i];
    }
    for (int i = 0; i < K; ++i) taps_host[i] = (float)(t[i] / sum);
    return 0;
}

// shapes every entry point takes; *grid: workgroups of one launch
static int gs_check_shape(int64_t planes, int H, int W, int K, int* grid, GaussArgs& a) {
    if (planes < 1 || H < 1 || W < 1 || K < 1 || K > SISR_GAUSS_MAX_K || K % 2 == 0) return SISR_E_BADARG;
    if (H <= K / 2 || W <= K / 2) return SISR_E_UNSUPPORTED;
    a.H = H; a.W = W; a.K = K;
    a.tiles_y = (H + GS_TH - 1) / GS_TH;
    a.tiles_x = (W + GS_TW - 1) / GS_TW;
    const int64_t tiles = (int64_t)a.tiles_y * a.tiles_x;                  // at most 2^57: no overflow
    if ((int64_t)H * W > INT32_MAX || planes > INT32_MAX / tiles) return SISR_E_TOOBIG;
    *grid = (int)(planes * tiles);
    return 0;
}

// do the byte ranges [p, p + n) and [q, q + m) share a byte (a NULL pointer shares none)
static bool gs_overlap(const void* p, int64_t n, const void* q, int64_t m) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return p && q && a < b + (uintptr_t)m && b < a + (uintptr_t)n;
}

template <int MODE>
static int gs_launch(const GaussArgs& a, int grid, hipStream_t st) {
    return sisr_launch<gauss_tile_kernel<MODE>>(dim3((unsigned)grid), dim3(SISR_BLOCK), gs_lds_bytes(a.K), SISR_LDS_BASE_DEFAULT, st, a);
}

template <int MODE>
static int gs_blur(const float* x, const float* taps_dev, float* y, int64_t planes, int H, int W, int K, void* stream) {
    GaussArgs a = {};
    int grid = 0;
    if (!x || !taps_dev || !y) return SISR_E_BADARG;
    if (int e = gs_check_shape(planes, H, W, K, &grid, a)) return e;
    const int64_t bytes = 4 * planes * H * W;             // planes <= INT32_MAX and H W <= INT32_MAX here
    if (gs_overlap(y, bytes, x, bytes) || gs_overlap(y, bytes, taps_dev, 4 * K)) return SISR_E_BADARG;
    a.x = x; a.taps = taps_dev; a.y = y;
    return gs_launch<MODE>(a, grid, sisr_stream(stream));
}

extern "C" int sisr_gauss_blur_fwd(const float* x, const float* taps_dev, float* y, int64_t planes, int32_t H, int32_t W, int32_t K,
                                   void* stream) {
    return gs_blur<GS_FWD>(x, taps_dev, y, planes, H, W, K, stream);
}

extern "C" int sisr_gauss_blur_bwd(const float* dy, const float* taps_dev, float* dx, int64_t planes, int32_t H, int32_t W, int32_t K,
                                   void* stream) {
    return gs_blur<GS_BWD>(dy, taps_dev, dx, planes, H, W, K, stream);
}

extern "C" int64_t sisr_usm_ws_bytes(int64_t planes, int32_t H, int32_t W) {
    if (planes < 1 || H < 1 || W < 1) return SISR_E_BADARG;
    if ((int64_t)H * W > INT32_MAX || planes > INT64_MAX / 5 / ((int64_t)H * W)) return SISR_E_TOOBIG;
    return 5 * planes * H * W;                            // a float (blur) and a byte (mask) per element
}

extern "C" int sisr_usm_fwd(const float* x, const float* taps_dev, int32_t K, float weight, float threshold, float lo, float hi, void* ws,
                            float* y, uint8_t* mask_out, int64_t planes, int32_t H, int32_t W, void* stream) {
    GaussArgs a = {};
    int grid = 0;
    if (!x || !taps_dev || !ws || !y) return SISR_E_BADARG;
    if (!(lo < hi) || std::isinf(lo) || std::isinf(hi) || !std::isfinite(weight) || !std::isfinite(threshold)) return SISR_E_BADARG;
    if (int e = gs_check_shape(planes, H, W, K, &grid, a)) return e;
    const int64_t ws_bytes = sisr_usm_ws_bytes(planes, H, W);
    if (ws_bytes < 0) return (int)ws_bytes;
    // what is written (y, ws, mask_out) shares no byte with what is read (x, the taps) nor with another output
    const int64_t n = ws_bytes / 5;
    const void* out[3] = {y, ws, mask_out};
    const int64_t out_bytes[3] = {4 * n, ws_bytes, n};
    for (int i = 0; i < 3; ++i) {
        if (gs_overlap(out[i], out_bytes[i], x, 4 * n) || gs_overlap(out[i], out_bytes[i], taps_dev, 4 * K)) return SISR_E_BADARG;
        for (int j = i + 1; j < 3; ++j)
            if (gs_overlap(out[i], out_bytes[i], out[j], out_bytes[j])) return SISR_E_BADARG;
    }
    a.x = x; a.taps = taps_dev; a.y = y;
    a.blur = (float*)ws;
    a.mask = (uint8_t*)ws + 4 * n;
    a.m = a.mask;
    a.mask_out = mask_out;
    a.weight = weight; a.threshold = threshold; a.lo = lo; a.hi = hi;
    a.scale = (float)(255.0 / ((double)hi - (double)lo));
    hipStream_t st = sisr_stream(stream);
    if (int e = gs_launch<GS_USM_MASK>(a, grid, st)) return e;
    return gs_launch<GS_USM_MIX>(a, grid, st);
}
