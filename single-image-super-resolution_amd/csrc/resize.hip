// resize.hip -- a differentiable fp32 image resize with torch's half-pixel coordinates (F.interpolate(..., align_corners=False) and
// mode='area'), forward and backward, the mode chosen PER SAMPLE from a table in device memory.
// Tensors are fp32 [N][C][H][W] -> [N][C][h][w], contiguous; a plane is one (n, c).  The operator is separable, y = R_h x R_w^T, and a
// row of R is defined in INTEGER arithmetic by rz_tap below (nothing depends on an fp32 scale): one __host__ __device__ text that the
// kernels, the host table (sisr_resize_taps_host) and the host's LDS plans all call.
//   resize_fwd_kernel  a workgroup owns an RZ_TH x RZ_TW (or smaller) tile of one output plane: the taps of the tile's rows and columns
//                      are computed once into LDS, the input footprint is staged with coalesced loads, filtered along x into LDS and
//                      along y out of it into one coalesced store.
//   resize_bwd_kernel  dx = R_h^T dy R_w in gather form: a workgroup owns a tile of one INPUT plane, finds the outputs that read it
//                      (rz_reach_lo / rz_reach_hi: a closed-form guess and a bounded walk over the monotone tap ranges), stages that
//                      block of dy and the outputs' taps in LDS and runs the two transposed passes.  Fixed order, no atomics, every
//                      element of dx stored: the same bits on every call.
// The mode is uniform within a workgroup (one plane) and is branched on once (the passes are templates).  The host does not know it,
// so the tile and the LDS plan are sized for the worst of the three modes at that ratio and halved until they fit RZ_LDS_BUDGET.
// Mode draw: Philox4x32-10 keyed by the seed (sisr_philox.h), word 3 of the counter DRAW_TAG_MODE | rank.  Plain vector stores only.
#include "sisr_dev.h"
#include "sisr_philox.h"
#include "sisr_cubic.h"

#include <algorithm>
#include <cmath>

#define RZ_TH 16
#define RZ_TW 64
#define RZ_LDS_BUDGET (64 * 1024)
static_assert(RZ_TH + RZ_TW <= SISR_BLOCK, "one thread per row and column of a tile computes its taps");
static_assert((RZ_TW & (RZ_TW - 1)) == 0 && (RZ_TH & (RZ_TH - 1)) == 0, "tiles are halved");

enum { RZ_AREA = SISR_RESIZE_AREA, RZ_BILINEAR = SISR_RESIZE_BILINEAR, RZ_BICUBIC = SISR_RESIZE_BICUBIC };

// ---- one row of R ---------------------------------------------------------------------------------------------------------------
// weights w[0 .. count - 1] on the UNCLAMPED input indices first .. first + count - 1 (area: w[0] on every one of them); a reader
// clamps the indices to 0 .. n_in - 1, and taps that clamp onto the same pixel add
struct RzTap {
    int first, count;
    float w[4];
};

// the polynomials of sisr_cubic.h (cc1, cc2: fp32, device only) for host and device, in DOUBLE and rounded once: evaluated in fp32,
// cc2's intermediate values of about 6 leave an absolute error of 3e-7 in a weight of 0.1.  Nothing here is contracted into fused
// multiply-adds, so the host's table holds the device's bits
__host__ __device__ static inline double rz_cc1(double x) {
#pragma clang fp contract(off)
    return (((double)CUBIC_A + 2.0) * x - ((double)CUBIC_A + 3.0)) * x * x + 1.0;
}
__host__ __device__ static inline double rz_cc2(double x) {
#pragma clang fp contract(off)
    return (((double)CUBIC_A * x - 5.0 * (double)CUBIC_A) * x + 8.0 * (double)CUBIC_A) * x - 4.0 * (double)CUBIC_A;
}

__host__ __device__ static inline RzTap rz_tap(int mode, int n_in, int n_out, int o) {
#pragma clang fp contract(off)
    RzTap t;
    t.w[1] = t.w[2] = t.w[3] = 0.f;
    if (mode == RZ_AREA) {
        const int64_t s = (int64_t)o * n_in / n_out;
        const int64_t e = ((int64_t)(o + 1) * n_in + n_out - 1) / n_out;
        t.first = (int)s;
        t.count = (int)(e - s);
        t.w[0] = 1.f / (float)t.count;
        return t;
    }
    const int64_t den = 2 * (int64_t)n_out;
    int64_t num = (2 * (int64_t)o + 1) * n_in - n_out;
    if (mode == RZ_BILINEAR && num < 0) num = 0;
    int64_t i0 = num / den;
    if (num < 0 && i0 * den != num) --i0;                                  // floor
    if (mode == RZ_BILINEAR) {
        const float f = (float)(num - i0 * den) / (float)den;
        t.first = (int)i0;
        t.count = 2;
        t.w[0] = 1.f - f;
        t.w[1] = f;
    } else {                                                               // bicubic, and every mode value outside 0 .. 2
        const double f = (double)(num - i0 * den) / (double)den;
        t.first = (int)i0 - 1;
        t.count = 4;
        t.w[0] = (float)rz_cc2(f + 1.0);
        t.w[1] = (float)rz_cc1(f);
        t.w[2] = (float)rz_cc1(1.0 - f);
        t.w[3] = (float)rz_cc2(2.0 - f);
    }
    return t;
}

__host__ __device__ static inline int rz_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the first and the last input index that output o reads (clamped); both are non-decreasing in o
__host__ __device__ static inline int rz_idx_lo(int mode, int n_in, int n_out, int o) {
    return rz_clamp(rz_tap(mode, n_in, n_out, o).first, 0, n_in - 1);
}
__host__ __device__ static inline int rz_idx_hi(int mode, int n_in, int n_out, int o) {
    const RzTap t = rz_tap(mode, n_in, n_out, o);
    return rz_clamp(t.first + t.count - 1, 0, n_in - 1);
}

// The outputs that read input index i are the run rz_reach_lo .. rz_reach_hi (empty when lo > hi: a down-scaling bilinear or bicubic
// skips pixels).  lo = the smallest o in 0 .. n_out with rz_idx_hi(o) >= i (n_out: none), hi = the largest o in -1 .. n_out - 1 with
// rz_idx_lo(o) <= i.  The guess is the output whose centre lies `reach` input pixels before (behind) the pixel, one index further
// out; the two walks make the answer exact whatever the guess, and they are short: at most about n_out / n_in + 3 steps.
__host__ __device__ static inline int rz_reach_lo(int mode, int n_in, int n_out, int i) {
    const int reach = mode == RZ_AREA ? 0 : (mode == RZ_BILINEAR ? 1 : 2);
    const int64_t g = (int64_t)(i - reach) * n_out / n_in - 1;
    int o = (int)(g < 0 ? 0 : (g > n_out - 1 ? n_out - 1 : g));
    while (o > 0 && rz_idx_hi(mode, n_in, n_out, o - 1) >= i) --o;
    while (o < n_out && rz_idx_hi(mode, n_in, n_out, o) < i) ++o;
    return o;
}
__host__ __device__ static inline int rz_reach_hi(int mode, int n_in, int n_out, int i) {
    const int reach = mode == RZ_AREA ? 0 : (mode == RZ_BILINEAR ? 1 : 2);
    const int64_t g = ((int64_t)(i + reach + 1) * n_out + n_in - 1) / n_in + 1;
    int o = (int)(g < 0 ? 0 : (g > n_out - 1 ? n_out - 1 : g));
    while (o < n_out - 1 && rz_idx_lo(mode, n_in, n_out, o + 1) <= i) ++o;
    while (o >= 0 && rz_idx_lo(mode, n_in, n_out, o) > i) --o;
    return o;
}

// ---- kernels --------------------------------------------------------------------------------------------------------------------
struct RzArgs {
    const float* src;        // forward: x [planes][H][W]; backward: dy [planes][h][w]
    const int* modes;        // [N], device memory
    float* dst;              // forward: y; backward: dx
    int C, H, W, h, w;       // H x W is the forward's input, h x w its output, in both kernels
    int TH, TW, lgTW;        // the tile (forward: of y, backward: of dx); powers of two
    int tiles_y, tiles_x;
    int SH, SW;              // the host's plan: rows and columns of the largest staged block over all tiles and modes
};

// words of LDS: the tile's tap tables, the staged block (odd pitch), the first pass's result
static inline int64_t rz_fwd_lds_words(int TH, int TW, int SH, int SW) { return 6 * (int64_t)(TH + TW) + (int64_t)SH * (SW | 1) + (int64_t)SH * TW; }
static inline int64_t rz_bwd_lds_words(int TH, int TW, int SH, int SW) {
    return 2 * (int64_t)(TH + TW) + 5 * ((int64_t)SH + SW) + (int64_t)SH * (SW | 1) + (int64_t)SH * TW;
}

// one output of a pass: the taps (first f, count n, weights wt) over `v` with stride `st`; `org` is the index of v[0], `last` the
// axis' last index.  The products (exact: 24 x 24 bits) are added in DOUBLE and the sum is rounded once per pass: with dyadic weights
// and operands the result is the exact one, rounded, where an fp32 chain would round at every tap (bicubic at ratio 1/2 has weights
// k / 256: the second pass carries 27 bits).  The vector unit runs fp64 fused multiply-adds at the fp32 rate, and the passes wait on LDS
template <int MODE>
__device__ __forceinline__ float rz_apply(const float* v, int st, int org, int last, int f, int n, const float* wt) {
    double acc = 0.0;
    if (MODE == RZ_AREA) {                                                 // the window lies inside the axis: no clamp
        const float* p = v + (f - org) * st;
        for (int k = 0; k < n; ++k) acc += (double)p[k * st];
        return (float)(acc * (double)wt[0]);
    }
    constexpr int CNT = MODE == RZ_BILINEAR ? 2 : 4;
#pragma unroll
    for (int k = 0; k < CNT; ++k) acc = fma((double)wt[k], (double)v[(rz_clamp(f + k, 0, last) - org) * st], acc);
    return (float)acc;
}

template <int MODE>
__device__ __forceinline__ void rz_fwd_passes(const RzArgs& a, const float* xs, float* tmp, float* dst, int P, int fy0, int fx0, int fh,
                                              int th, int tw, int oy0, int ox0, const int* yf, const int* yc, const float* yw,
                                              const int* xf, const int* xc, const float* xw) {
    const int tid = threadIdx.x, TW = a.TW;
    // along x: tmp[r][c] for every staged row r and tile column c; lanes on consecutive columns
    for (int i = tid; i < fh * TW; i += SISR_BLOCK) {
        const int r = i >> a.lgTW, c = i & (TW - 1);
        if (c < tw) tmp[r * TW + c] = rz_apply<MODE>(xs + r * P, 1, fx0, a.W - 1, xf[c], xc[c], xw + 4 * c);
    }
    __syncthreads();
    // along y, out of LDS into one coalesced store
    for (int i = tid; i < th * TW; i += SISR_BLOCK) {
        const int r = i >> a.lgTW, c = i & (TW - 1);
        if (c < tw) dst[(size_t)(oy0 + r) * a.w + (ox0 + c)] = rz_apply<MODE>(tmp + c, TW, fy0, a.H - 1, yf[r], yc[r], yw + 4 * r);
    }
}

__global__ void __launch_bounds__(SISR_BLOCK) resize_fwd_kernel(RzArgs a) {
    extern __shared__ float rz_lds[];
    const int tid = threadIdx.x;
    const int tiles = a.tiles_x * a.tiles_y;
    const int plane = blockIdx.x / tiles, t = blockIdx.x - plane * tiles;
    const int ty = t / a.tiles_x, tx = t - ty * a.tiles_x;
    const int oy0 = ty * a.TH, ox0 = tx * a.TW;
    const int th = min(a.TH, a.h - oy0), tw = min(a.TW, a.w - ox0);
    int mode = a.modes[plane / a.C];
    if ((unsigned)mode > 2u) mode = RZ_BICUBIC;
    int* yf = reinterpret_cast<int*>(rz_lds);                              // [TH] first, [TH] count, [TH][4] weights; then the columns'
    int* yc = yf + a.TH;
    float* yw = reinterpret_cast<float*>(yc + a.TH);
    int* xf = reinterpret_cast<int*>(yw + 4 * a.TH);
    int* xc = xf + a.TW;
    float* xw = reinterpret_cast<float*>(xc + a.TW);
    float* xs = xw + 4 * a.TW;                                             // [SH][P]
    const int P = a.SW | 1;
    float* tmp = xs + a.SH * P;                                            // [SH][TW]

    if (tid < th + tw) {
        const bool is_y = tid < th;
        const int j = is_y ? tid : tid - th;
        const RzTap tp = is_y ? rz_tap(mode, a.H, a.h, oy0 + j) : rz_tap(mode, a.W, a.w, ox0 + j);
        (is_y ? yf : xf)[j] = tp.first;
        (is_y ? yc : xc)[j] = tp.count;
        float* wd = (is_y ? yw : xw) + 4 * j;
        wd[0] = tp.w[0]; wd[1] = tp.w[1]; wd[2] = tp.w[2]; wd[3] = tp.w[3];
    }
    __syncthreads();
    // the footprint: first and count are non-decreasing along the tile.  The host's plan covers it for every mode (the min is never taken)
    const int fy0 = rz_clamp(yf[0], 0, a.H - 1), fx0 = rz_clamp(xf[0], 0, a.W - 1);
    const int fh = min(rz_clamp(yf[th - 1] + yc[th - 1] - 1, 0, a.H - 1) - fy0 + 1, a.SH);
    const int fw = min(rz_clamp(xf[tw - 1] + xc[tw - 1] - 1, 0, a.W - 1) - fx0 + 1, a.SW);
    const float* src = a.src + (size_t)plane * (size_t)a.H * (size_t)a.W + (size_t)fy0 * a.W + fx0;
    if (fw >= 32) {                                                        // a wave per row
        for (int r = tid >> 6; r < fh; r += SISR_BLOCK / 64)
            for (int c = tid & 63; c < fw; c += 64) xs[r * P + c] = src[(size_t)r * a.W + c];
    } else {
        for (int i = tid; i < fh * fw; i += SISR_BLOCK) {
            const int r = i / fw, c = i - r * fw;
            xs[r * P + c] = src[(size_t)r * a.W + c];
        }
    }
    __syncthreads();
    float* dst = a.dst + (size_t)plane * (size_t)a.h * (size_t)a.w;
    if (mode == RZ_AREA) rz_fwd_passes<RZ_AREA>(a, xs, tmp, dst, P, fy0, fx0, fh, th, tw, oy0, ox0, yf, yc, yw, xf, xc, xw);
    else if (mode == RZ_BILINEAR) rz_fwd_passes<RZ_BILINEAR>(a, xs, tmp, dst, P, fy0, fx0, fh, th, tw, oy0, ox0, yf, yc, yw, xf, xc, xw);
    else rz_fwd_passes<RZ_BICUBIC>(a, xs, tmp, dst, P, fy0, fx0, fh, th, tw, oy0, ox0, yf, yc, yw, xf, xc, xw);
}

// the weight with which staged output j (first index f, weights wt) reads input index i: the taps that clamp onto i add, in tap order.
// Only outputs inside the pixel's reach are asked, so for area the answer is the window's one weight
template <int MODE>
__device__ __forceinline__ float rz_weight_of(int f, const float* wt, int i, int last) {
    if (MODE == RZ_AREA) return wt[0];
    constexpr int CNT = MODE == RZ_BILINEAR ? 2 : 4;
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < CNT; ++k) s += rz_clamp(f + k, 0, last) == i ? wt[k] : 0.f;
    return s;
}

template <int MODE>
__device__ __forceinline__ void rz_bwd_passes(const RzArgs& a, const float* gs, float* tmp, float* dst, int P, int oy_lo, int ox_lo, int sh,
                                              int th, int tw, int iy0, int ix0, const int* ylo, const int* yhi, const int* xlo,
                                              const int* xhi, const int* yf, const float* yw, const int* xf, const float* xw) {
    const int tid = threadIdx.x, TW = a.TW;
    // along x: tmp[r][c] = sum over the outputs o that read column ix0 + c of R_w[o][ix0 + c] dy[r][o], in the order of o
    for (int i = tid; i < sh * TW; i += SISR_BLOCK) {
        const int r = i >> a.lgTW, c = i & (TW - 1);
        if (c >= tw) continue;
        float acc = 0.f;
        for (int o = xlo[c]; o <= xhi[c]; ++o) {
            const int j = o - ox_lo;
            acc = fmaf(rz_weight_of<MODE>(xf[j], xw + 4 * j, ix0 + c, a.W - 1), gs[r * P + j], acc);
        }
        tmp[r * TW + c] = acc;
    }
    __syncthreads();
    for (int i = tid; i < th * TW; i += SISR_BLOCK) {
        const int r = i >> a.lgTW, c = i & (TW - 1);
        if (c >= tw) continue;
        float acc = 0.f;
        for (int o = ylo[r]; o <= yhi[r]; ++o) {
            const int j = o - oy_lo;
            acc = fmaf(rz_weight_of<MODE>(yf[j], yw + 4 * j, iy0 + r, a.H - 1), tmp[j * TW + c], acc);
        }
        dst[(size_t)(iy0 + r) * a.W + (ix0 + c)] = acc;
    }
}

__global__ void __launch_bounds__(SISR_BLOCK) resize_bwd_kernel(RzArgs a) {
    extern __shared__ float rz_lds[];
    const int tid = threadIdx.x;
    const int tiles = a.tiles_x * a.tiles_y;
    const int plane = blockIdx.x / tiles, t = blockIdx.x - plane * tiles;
    const int ty = t / a.tiles_x, tx = t - ty * a.tiles_x;
    const int iy0 = ty * a.TH, ix0 = tx * a.TW;
    const int th = min(a.TH, a.H - iy0), tw = min(a.TW, a.W - ix0);
    int mode = a.modes[plane / a.C];
    if ((unsigned)mode > 2u) mode = RZ_BICUBIC;
    int* ylo = reinterpret_cast<int*>(rz_lds);                             // [TH] lo, [TH] hi, [TW] lo, [TW] hi: the reach of the tile's pixels
    int* yhi = ylo + a.TH;
    int* xlo = yhi + a.TH;
    int* xhi = xlo + a.TW;
    int* yf = xhi + a.TW;                                                  // [SH] first, [SH][4] weights of the staged outputs; then the columns'
    float* yw = reinterpret_cast<float*>(yf + a.SH);
    int* xf = reinterpret_cast<int*>(yw + 4 * a.SH);
    float* xw = reinterpret_cast<float*>(xf + a.SW);
    float* gs = xw + 4 * a.SW;                                             // [SH][P]
    const int P = a.SW | 1;
    float* tmp = gs + a.SH * P;                                            // [SH][TW]

    if (tid < th + tw) {
        const bool is_y = tid < th;
        const int j = is_y ? tid : tid - th;
        const int n_in = is_y ? a.H : a.W, n_out = is_y ? a.h : a.w, i = (is_y ? iy0 : ix0) + j;
        (is_y ? ylo : xlo)[j] = rz_reach_lo(mode, n_in, n_out, i);
        (is_y ? yhi : xhi)[j] = rz_reach_hi(mode, n_in, n_out, i);
    }
    __syncthreads();
    // lo and hi are non-decreasing along the tile: the block of dy that the tile gathers.  The host's plan covers it for every mode
    const int oy_lo = ylo[0], ox_lo = xlo[0];
    const int sh = min(yhi[th - 1] - oy_lo + 1, a.SH), sw = min(xhi[tw - 1] - ox_lo + 1, a.SW);
    float* dst = a.dst + (size_t)plane * (size_t)a.H * (size_t)a.W;
    if (sh <= 0 || sw <= 0) {                                              // nobody reads these pixels
        for (int i = tid; i < th * a.TW; i += SISR_BLOCK) {
            const int r = i >> a.lgTW, c = i & (a.TW - 1);
            if (c < tw) dst[(size_t)(iy0 + r) * a.W + (ix0 + c)] = 0.f;
        }
        return;
    }
    for (int i = tid; i < sh + sw; i += SISR_BLOCK) {
        const bool is_y = i < sh;
        const int j = is_y ? i : i - sh;
        const RzTap tp = is_y ? rz_tap(mode, a.H, a.h, oy_lo + j) : rz_tap(mode, a.W, a.w, ox_lo + j);
        (is_y ? yf : xf)[j] = tp.first;
        float* wd = (is_y ? yw : xw) + 4 * j;
        wd[0] = tp.w[0]; wd[1] = tp.w[1]; wd[2] = tp.w[2]; wd[3] = tp.w[3];
    }
    const float* src = a.src + (size_t)plane * (size_t)a.h * (size_t)a.w + (size_t)oy_lo * a.w + ox_lo;
    if (sw >= 32) {
        for (int r = tid >> 6; r < sh; r += SISR_BLOCK / 64)
            for (int c = tid & 63; c < sw; c += 64) gs[r * P + c] = src[(size_t)r * a.w + c];
    } else {
        for (int i = tid; i < sh * sw; i += SISR_BLOCK) {
            const int r = i / sw, c = i - r * sw;
            gs[r * P + c] = src[(size_t)r * a.w + c];
        }
    }
    __syncthreads();
    if (mode == RZ_AREA) rz_bwd_passes<RZ_AREA>(a, gs, tmp, dst, P, oy_lo, ox_lo, sh, th, tw, iy0, ix0, ylo, yhi, xlo, xhi, yf, yw, xf, xw);
    else if (mode == RZ_BILINEAR) rz_bwd_passes<RZ_BILINEAR>(a, gs, tmp, dst, P, oy_lo, ox_lo, sh, th, tw, iy0, ix0, ylo, yhi, xlo, xhi, yf, yw, xf, xw);
    else rz_bwd_passes<RZ_BICUBIC>(a, gs, tmp, dst, P, oy_lo, ox_lo, sh, th, tw, iy0, ix0, ylo, yhi, xlo, xhi, yf, yw, xf, xw);
}

// ---- the mode draw ----------------------------------------------------------------------------------------------------------------
struct RzDrawArgs {
    uint64_t seed;
    int rank, B;
    float p[3];              // normalised: see rz_draw_args
};

// draw_pick over the three weights on u0 = draw_uniform(r0)
__host__ __device__ __forceinline__ int rz_draw_mode(const RzDrawArgs& a, int64_t t, int b) {
    uint32_t r[4];
    draw_words(a.seed, t, (uint32_t)b, DRAW_TAG_MODE | (uint32_t)a.rank, r);
    return draw_pick(a.p, 3, draw_uniform(r[0]));
}

// checks, and divides the three weights by their fp32 sum (p0 + p1) + p2
static bool rz_draw_args(uint64_t seed, int rank, int B, float p0, float p1, float p2, RzDrawArgs& a) {
    const float p[3] = {p0, p1, p2};
    if (B < 1 || rank < 0 || rank >= DRAW_RANK_LIMIT) return false;
    for (int i = 0; i < 3; ++i)
        if (!std::isfinite(p[i]) || p[i] < 0.f) return false;
    const float s = (p0 + p1) + p2;
    if (!(s > 0.f) || !std::isfinite(s)) return false;
    a.seed = seed; a.rank = rank; a.B = B;
    for (int i = 0; i < 3; ++i) a.p[i] = p[i] / s;
    return true;
}

// One workgroup; the step is only read (the launch shares the step that the stage's draw stored)
__global__ void __launch_bounds__(SISR_BLOCK) resize_modes_kernel(const int64_t* __restrict__ drawn_step, RzDrawArgs a, int* __restrict__ modes) {
    const int64_t t = *drawn_step;
    for (int b = threadIdx.x; b < a.B; b += SISR_BLOCK) modes[b] = rz_draw_mode(a, t, b);
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
struct RzPlan {
    int TH, TW, lgTW, SH, SW;
    int64_t words;           // of LDS; above the budget: the shape is refused
};

// rows (columns) of the largest block that a tile of T consecutive indices of the tiled axis stages, over all tiles and the three modes
template <bool BWD>
static int rz_axis_span(int T, int n_in, int n_out) {
    const int n_tiled = BWD ? n_in : n_out;
    int span = 1;
    for (int64_t j0 = 0; j0 < n_tiled; j0 += T) {
        const int j1 = (int)std::min<int64_t>(j0 + T, n_tiled) - 1;
        for (int mode = 0; mode < 3; ++mode) {
            const int lo = BWD ? rz_reach_lo(mode, n_in, n_out, (int)j0) : rz_idx_lo(mode, n_in, n_out, (int)j0);
            const int hi = BWD ? rz_reach_hi(mode, n_in, n_out, j1) : rz_idx_hi(mode, n_in, n_out, j1);
            span = std::max(span, hi - lo + 1);
        }
    }
    return span;
}

template <bool BWD>
static RzPlan rz_plan(int H, int W, int h, int w) {
    RzPlan p;
    p.TH = RZ_TH; p.TW = RZ_TW;
    for (;;) {
        p.SH = rz_axis_span<BWD>(p.TH, H, h);
        p.SW = rz_axis_span<BWD>(p.TW, W, w);
        p.words = BWD ? rz_bwd_lds_words(p.TH, p.TW, p.SH, p.SW) : rz_fwd_lds_words(p.TH, p.TW, p.SH, p.SW);
        if (4 * p.words <= RZ_LDS_BUDGET || (p.TH == 1 && p.TW == 1)) break;
        if (p.TW > 1 && (p.SW >= p.SH || p.TH == 1)) p.TW >>= 1;         // halve the axis with the longer staged side
        else p.TH >>= 1;
    }
    p.lgTW = 0;
    while ((1 << p.lgTW) < p.TW) ++p.lgTW;
    return p;
}

// both plans of a shape; the latest shape's are kept (a training step asks for the same few shapes over and over)
struct RzPlans {
    int H, W, h, w;
    RzPlan fwd, bwd;
};
static const RzPlans& rz_plans(int H, int W, int h, int w) {
    static thread_local RzPlans last[4] = {};
    static thread_local int next = 0;
    for (const RzPlans& p : last)
        if (p.H == H && p.W == W && p.h == h && p.w == w) return p;
    RzPlans& p = last[next];
    next = (next + 1) & 3;
    p.H = H; p.W = W; p.h = h; p.w = w;
    p.fwd = rz_plan<false>(H, W, h, w);
    p.bwd = rz_plan<true>(H, W, h, w);
    return p;
}

static bool rz_overlap(const void* p, int64_t n, const void* q, int64_t m) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + (uintptr_t)m && b < a + (uintptr_t)n;
}

template <bool BWD>
static int rz_run(const float* src, const int32_t* modes, float* dst, int32_t N, int32_t C, int32_t H, int32_t W, int32_t h, int32_t w,
                  void* stream) {
    if (!src || !modes || !dst || N < 1 || C < 1 || H < 1 || W < 1 || h < 1 || w < 1) return SISR_E_BADARG;
    const int64_t planes = (int64_t)N * C;
    if ((int64_t)H * W > INT32_MAX || (int64_t)h * w > INT32_MAX || planes > INT32_MAX) return SISR_E_TOOBIG;
    const int64_t big = 4 * planes * H * W, small = 4 * planes * h * w;   // at most 2^64 / 4: planes, H W and h w are below 2^31
    if (rz_overlap(src, BWD ? small : big, dst, BWD ? big : small) || rz_overlap(modes, 4 * (int64_t)N, dst, BWD ? big : small))
        return SISR_E_BADARG;
    const RzPlans& pl = rz_plans(H, W, h, w);
    if (4 * pl.fwd.words > RZ_LDS_BUDGET || 4 * pl.bwd.words > RZ_LDS_BUDGET) return SISR_E_UNSUPPORTED;    // both directions refuse the same shapes
    const RzPlan& p = BWD ? pl.bwd : pl.fwd;
    RzArgs a = {};
    a.src = src; a.modes = modes; a.dst = dst;
    a.C = C; a.H = H; a.W = W; a.h = h; a.w = w;
    a.TH = p.TH; a.TW = p.TW; a.lgTW = p.lgTW; a.SH = p.SH; a.SW = p.SW;
    a.tiles_y = ((BWD ? H : h) + p.TH - 1) / p.TH;
    a.tiles_x = ((BWD ? W : w) + p.TW - 1) / p.TW;
    const int64_t tiles = (int64_t)a.tiles_y * a.tiles_x;                  // at most H W (h w) <= INT32_MAX
    if (planes > INT32_MAX / tiles) return SISR_E_TOOBIG;
    const dim3 grid((unsigned)(planes * tiles));
    if (BWD) return sisr_launch<resize_bwd_kernel>(grid, dim3(SISR_BLOCK), (int)(4 * p.words), SISR_LDS_BASE_DEFAULT, sisr_stream(stream), a);
    return sisr_launch<resize_fwd_kernel>(grid, dim3(SISR_BLOCK), (int)(4 * p.words), SISR_LDS_BASE_DEFAULT, sisr_stream(stream), a);
}

extern "C" int sisr_resize_fwd(const float* x, const int32_t* modes_dev, float* y, int32_t N, int32_t C, int32_t H, int32_t W, int32_t h,
                               int32_t w, void* stream) {
    return rz_run<false>(x, modes_dev, y, N, C, H, W, h, w, stream);
}

extern "C" int sisr_resize_bwd(const float* dy, const int32_t* modes_dev, float* dx, int32_t N, int32_t C, int32_t H, int32_t W, int32_t h,
                               int32_t w, void* stream) {
    return rz_run<true>(dy, modes_dev, dx, N, C, H, W, h, w, stream);
}

extern "C" int sisr_resize_taps_host(int32_t mode, int32_t n_in, int32_t n_out, int32_t* first, int32_t* count, float* w) {
    if (!first || !count || !w || mode < 0 || mode > 2 || n_in < 1 || n_out < 1) return SISR_E_BADARG;
    for (int o = 0; o < n_out; ++o)
        if (rz_tap(mode, n_in, n_out, o).count > SISR_RESIZE_MAX_TAPS) return SISR_E_UNSUPPORTED;
    for (int o = 0; o < n_out; ++o) {
        const RzTap t = rz_tap(mode, n_in, n_out, o);
        first[o] = t.first;
        count[o] = t.count;
        float* row = w + (int64_t)o * SISR_RESIZE_MAX_TAPS;
        for (int k = 0; k < SISR_RESIZE_MAX_TAPS; ++k) row[k] = k < t.count ? t.w[mode == RZ_AREA ? 0 : k] : 0.f;
    }
    return 0;
}

extern "C" int sisr_resize_modes_draw(const int64_t* drawn_step_dev, uint64_t seed, int32_t rank, int32_t B, float p_area, float p_bilinear,
                                      float p_bicubic, int32_t* modes_dev, void* stream) {
    RzDrawArgs a;
    if (!drawn_step_dev || !modes_dev || !rz_draw_args(seed, rank, B, p_area, p_bilinear, p_bicubic, a)) return SISR_E_BADARG;
    hipLaunchKernelGGL(resize_modes_kernel, dim3(1), dim3(SISR_BLOCK), 0, sisr_stream(stream), drawn_step_dev, a, modes_dev);
    SISR_CHECK_LAUNCH();
    return 0;
}

extern "C" int sisr_resize_modes_host(int64_t t, uint64_t seed, int32_t rank, int32_t B, float p_area, float p_bilinear, float p_bicubic,
                                      int32_t* modes_host) {
    RzDrawArgs a;
    if (!modes_host || t < 0 || !rz_draw_args(seed, rank, B, p_area, p_bilinear, p_bicubic, a)) return SISR_E_BADARG;
    for (int b = 0; b < B; ++b) modes_host[b] = rz_draw_mode(a, t, b);
    return 0;
}
