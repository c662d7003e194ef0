// tiles.hip -- whole-image super-resolution in tiles: an image of any size is cut into overlapping windows of
// one shape, the generator runs over them as an ordinary batch, and the SR tiles are put together again.
//   sisr_tile_axis         HOST: the plan of one axis -- window origins a_i and ownership boundaries b_i;
//   tile_gather_f32_kernel the fp32 counterpart of patch_gather_kernel (patchsrc.hip): windows of ONE normalised [C][H][W] image ->
//                          [n][C][th][tw], through LDS so that reads and writes are both coalesced for all eight operations;
//   tile_stitch_kernel     output-centric: one thread per output pixel finds the tiles that carry weight there, undoes each
//                          member's flips / transposition and sums in a fixed order.  No atomics, plain vector stores: the same
//                          bits on every call, capturable.
// The same table rows (index, y0, x0, ops) drive sisr_patch_gather, the fp32 gather and the stitch.  Neither kernel trusts device
// tables: every origin is clamped into its image and every tile coordinate into its tile.
#include "sisr_dev.h"

#include <algorithm>

// ---- the plan of one axis ----------------------------------------------------------------------------------------------------------
extern "C" int sisr_tile_axis(int32_t L, int32_t T, int32_t halo, int32_t* a_out, int32_t* b_out, int32_t cap) {
    if (L < 1 || T < 1 || halo < 0 || (a_out == nullptr) != (b_out == nullptr) || (a_out && cap < 1)) return SISR_E_BADARG;
    if (L <= T) {
        if (a_out) { a_out[0] = 0; b_out[0] = L; }
        return 1;
    }
    const int64_t core = (int64_t)T - 2 * (int64_t)halo;
    if (core < 1) return SISR_E_BADARG;
    const int64_t n = ((int64_t)L - 2 * (int64_t)halo + core - 1) / core;       // >= 2: L - 2 halo > T - 2 halo = core
    if (!a_out) return (int)n;                                                  // n <= L: fits
    if (n > cap) return SISR_E_TOOBIG;
    for (int64_t i = 0; i < n; ++i) a_out[i] = (int32_t)std::min<int64_t>(i * core, (int64_t)L - T);
    for (int64_t i = 0; i + 1 < n; ++i) b_out[i] = (int32_t)(((int64_t)a_out[i + 1] + a_out[i] + T) / 2);
    b_out[n - 1] = L;
    return (int)n;
}

// ---- fp32 gather -------------------------------------------------------------------------------------------------------------------
// patch_gather_kernel's tile walk with a float tile: TG_T x TG_T window pixels of one channel at a time; LDS pitch 33 dwords, so
// the transposed read (one row per lane) falls on 32 different banks.
#define TG_T 32
#define TG_PITCH (TG_T + 1)

__global__ void __launch_bounds__(SISR_BLOCK) tile_gather_f32_kernel(const float* __restrict__ src, int C, int H, int W,
                                                                      const int32_t* __restrict__ table, int h, int w,
                                                                      float* __restrict__ dst) {
    __shared__ float tile[TG_T * TG_PITCH];
    const int b = blockIdx.z;
    const int y0 = max(min(table[4 * b + 1], H - h), 0);                  // never outside the source, whatever the table holds
    const int x0 = max(min(table[4 * b + 2], W - w), 0);
    int ops = table[4 * b + 3] & 7;
    if (h != w) ops &= 3;
    const bool fh = ops & 1, fv = ops & 2, tr = ops & 4;
    const int ty0 = blockIdx.y * TG_T, tx0 = blockIdx.x * TG_T;           // tile origin inside the window
    const int th = min(TG_T, h - ty0), tw = min(TG_T, w - tx0);           // ragged last tiles
    // the tile after hflip, vflip: rows [yb, yb + th), columns [xb, xb + tw) of the flipped window; after the transposition its
    // rows are the flipped window's columns
    const int yb = fv ? h - ty0 - th : ty0, xb = fh ? w - tx0 - tw : tx0;
    const int OH = tr ? w : h, OW = tr ? h : w;
    const int on = tr ? tw : th, om = tr ? th : tw;                       // rows, columns of the destination tile
    const int oy0 = tr ? xb : yb, ox0 = tr ? yb : xb;
    const int q = threadIdx.x & (TG_T - 1);
    for (int c = 0; c < C; ++c) {
        const float* in = src + ((int64_t)c * H + y0 + ty0) * W + x0 + tx0;
        for (int i = threadIdx.x; i < th * tw; i += SISR_BLOCK) {
            const int r = i / tw, j = i - r * tw;
            tile[r * TG_PITCH + j] = in[(int64_t)r * W + j];
        }
        __syncthreads();
        float* out = dst + ((int64_t)b * C + c) * OH * OW;
        if (q < om) {
            for (int r = threadIdx.x / TG_T; r < on; r += SISR_BLOCK / TG_T) {
                const int ly = tr ? q : r, lx = tr ? r : q;
                const int lsy = fv ? th - 1 - ly : ly, lsx = fh ? tw - 1 - lx : lx;
                out[(int64_t)(oy0 + r) * OW + ox0 + q] = tile[lsy * TG_PITCH + lsx];
            }
        }
        __syncthreads();
    }
}

extern "C" int sisr_tile_gather_f32(const float* src, int32_t C, int32_t H, int32_t W, const int32_t* table_dev, int32_t n,
                                    int32_t th, int32_t tw, float* dst, void* stream) {
    if (!src || !table_dev || !dst || C < 1 || C > 4 || H < 1 || W < 1 || n < 1 || th < 1 || tw < 1 || th > H || tw > W)
        return SISR_E_BADARG;
    const int tiles_x = (tw + TG_T - 1) / TG_T, tiles_y = (th + TG_T - 1) / TG_T;
    if (n > 65535 || tiles_y > 65535) return SISR_E_TOOBIG;
    hipLaunchKernelGGL(tile_gather_f32_kernel, dim3(tiles_x, tiles_y, n), dim3(SISR_BLOCK), 0, sisr_stream(stream), src, C, H, W,
                       table_dev, th, tw, dst);
    SISR_CHECK_LAUNCH();
    return 0;
}

// ---- stitch ------------------------------------------------------------------------------------------------------------------------
// One axis at LR position p = (Y + 0.5) / s (never an integer).  Tile i carries weight where b[i-1] - f < p < b[i] + f; b ascends,
// so those tiles are one run [lo, hi]: lo is the first tile whose right ramp has not ended, hi the last whose left ramp has begun.
// f == 0: the run is the one tile that owns p.
__device__ __forceinline__ void stitch_axis_run(const int32_t* __restrict__ b, int n, float f, float p, int& lo, int& hi) {
    lo = 0;
    while (lo < n - 1 && (float)b[lo] + f <= p) ++lo;
    hi = lo;
    while (hi < n - 1 && p > (float)b[hi] - f) ++hi;
}

// raw weight r_i = clamp(min(dL, dR), 0, 1), dL = (p - (b[i-1] - f)) / 2f (first tile: +inf), dR = ((b[i] + f) - p) / 2f (last: +inf)
__device__ __forceinline__ float stitch_axis_raw(const int32_t* __restrict__ b, int n, float f, float p, int i) {
    if (f == 0.f) return 1.f;                                             // the owner (stitch_axis_run found it)
    float r = 1.f;
    if (i > 0) r = fminf(r, (p - ((float)b[i - 1] - f)) / (2.f * f));
    if (i < n - 1) r = fminf(r, (((float)b[i] + f) - p) / (2.f * f));
    return fmaxf(r, 0.f);
}

struct StitchArgs {
    const float* tiles;                    // [E * ny * nx][C][s th][s tw]
    const int32_t* table;                  // [E * ny * nx][4]: the ops of every row
    const int32_t *ay, *by, *ax, *bx;      // origins and ownership boundaries of the two axes
    int ny, nx, C, H, W, th, tw, s, E;
    float f, mean, stdv;
};

// KIND 0: dst [C][sH][sW] fp32; KIND 1: dst [sH][sW][C] uint8.  Thread = output pixel, 32 along X (one 128-byte fp32 row segment
// per half-wave) x 8 along Y.  Untransposed members are read along tile rows; a transposed member's reads walk down a tile column
// (32 lines per half-wave, re-used by the seven rows that follow out of L2): the generator forward in front of this launch outweighs
// it by orders of magnitude.
template <int KIND>
__global__ void __launch_bounds__(SISR_BLOCK) tile_stitch_kernel(StitchArgs a, void* __restrict__ dst) {
    const int X = blockIdx.x * 32 + (threadIdx.x & 31), Y = blockIdx.y * 8 + (threadIdx.x >> 5);
    const int sH = a.s * a.H, sW = a.s * a.W;
    if (X >= sW || Y >= sH) return;
    const float inv_s = 1.f / (float)a.s;                                 // s is a power of two: exact
    const float py = ((float)Y + 0.5f) * inv_s, px = ((float)X + 0.5f) * inv_s;
    int ylo, yhi, xlo, xhi;
    stitch_axis_run(a.by, a.ny, a.f, py, ylo, yhi);
    stitch_axis_run(a.bx, a.nx, a.f, px, xlo, xhi);
    float sum_y = 0.f, sum_x = 0.f;
    for (int i = ylo; i <= yhi; ++i) sum_y += stitch_axis_raw(a.by, a.ny, a.f, py, i);
    for (int i = xlo; i <= xhi; ++i) sum_x += stitch_axis_raw(a.bx, a.nx, a.f, px, i);
    const int hh = a.s * a.th, ww = a.s * a.tw;                           // an untransposed SR tile is hh x ww
    const int64_t plane = (int64_t)hh * ww;
    const int n = a.ny * a.nx;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    for (int e = 0; e < a.E; ++e) {
        float ve[4] = {0.f, 0.f, 0.f, 0.f};
        for (int iy = ylo; iy <= yhi; ++iy) {
            const float wy = stitch_axis_raw(a.by, a.ny, a.f, py, iy) / sum_y;
            const int oy = max(min(a.ay[iy], a.H - a.th), 0);             // clamped like the gathers: never outside a tile
            const int ly = max(min(Y - a.s * oy, hh - 1), 0);
            for (int ix = xlo; ix <= xhi; ++ix) {
                const float w = wy * (stitch_axis_raw(a.bx, a.nx, a.f, px, ix) / sum_x);
                const int ox = max(min(a.ax[ix], a.W - a.tw), 0);
                const int lx = max(min(X - a.s * ox, ww - 1), 0);
                const int64_t row = (int64_t)e * n + (int64_t)iy * a.nx + ix;
                int ops = a.table[4 * row + 3] & 7;
                if (a.th != a.tw) ops &= 3;
                // inverse of "hflip, vflip, transpose": the flipped coordinates, then rows and columns change places
                const int yf = (ops & 2) ? hh - 1 - ly : ly, xf = (ops & 1) ? ww - 1 - lx : lx;
                const int64_t at = (ops & 4) ? (int64_t)xf * hh + yf : (int64_t)yf * ww + xf;
                const float* t = a.tiles + row * a.C * plane + at;
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (c < a.C) {
                        const float tv = t[c * plane];
                        if (a.f == 0.f) ve[c] = tv;                       // one owner: copied, not multiplied
                        else ve[c] += w * tv;
                    }
            }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = a.E == 1 ? ve[c] : v[c] + ve[c];
    }
    const float inv_e = 1.f / (float)a.E;
#pragma unroll
    for (int c = 0; c < 4; ++c)
        if (c < a.C) {
            const float r = a.E == 1 ? v[c] : v[c] * inv_e;
            if (KIND == 0) {
                reinterpret_cast<float*>(dst)[((int64_t)c * sH + Y) * sW + X] = r;
            } else {
                // p = (v std + mean) 255, each operation rounded on its own; q = floor(p + 0.5) in [0, 255], NaN -> 0
                const float p = __fmul_rn(__fadd_rn(__fmul_rn(r, a.stdv), a.mean), 255.f);
                float qf = floorf(__fadd_rn(p, 0.5f));
                qf = qf >= 0.f ? fminf(qf, 255.f) : 0.f;                  // a NaN fails the comparison
                reinterpret_cast<unsigned char*>(dst)[((int64_t)Y * sW + X) * a.C + c] = (unsigned char)(int)qf;
            }
        }
}

extern "C" int sisr_tile_stitch(const float* tiles, const int32_t* table_dev, const int32_t* ay_dev, const int32_t* by_dev,
                                int32_t ny, const int32_t* ax_dev, const int32_t* bx_dev, int32_t nx, int32_t C, int32_t H,
                                int32_t W, int32_t th, int32_t tw, int32_t scale, int32_t halo, float feather, int32_t E,
                                float mean, float stdv, void* dst, int32_t dst_kind, void* stream) {
    if (!tiles || !table_dev || !ay_dev || !by_dev || !ax_dev || !bx_dev || !dst) return SISR_E_BADARG;
    if (ny < 1 || nx < 1 || H < 1 || W < 1 || th < 1 || tw < 1 || th > H || tw > W || C < 1 || C > 4) return SISR_E_BADARG;
    if (scale != 1 && scale != 2 && scale != 4 && scale != 8) return SISR_E_BADARG;
    if ((E != 1 && E != 8) || (E == 8 && th != tw)) return SISR_E_BADARG;
    if (halo < 0 || !(feather >= 0.f && feather <= (float)halo)) return SISR_E_BADARG;      // NaN included
    if (dst_kind != 0 && dst_kind != 1) return SISR_E_BADARG;
    if ((int64_t)E * ny * nx >= (int64_t)1 << 29 || H > 1 << 27 || W > 1 << 27) return SISR_E_TOOBIG;
    const int gx = (scale * W + 31) / 32, gy = (scale * H + 7) / 8;
    if (gy > 65535) return SISR_E_TOOBIG;
    const StitchArgs a = {tiles, table_dev, ay_dev, by_dev, ax_dev, bx_dev, ny, nx, C, H, W, th, tw, scale, E, feather, mean, stdv};
    if (dst_kind == 0)
        hipLaunchKernelGGL(tile_stitch_kernel<0>, dim3(gx, gy), dim3(SISR_BLOCK), 0, sisr_stream(stream), a, dst);
    else
        hipLaunchKernelGGL(tile_stitch_kernel<1>, dim3(gx, gy), dim3(SISR_BLOCK), 0, sisr_stream(stream), a, dst);
    SISR_CHECK_LAUNCH();
    return 0;
}
