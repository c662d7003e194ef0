// jpeg.hip -- a differentiable JPEG round trip y = J(x) on the device, forward and backward (the definition is
// pinned in sisr_hip.h): colour transform, edge-replication pad to the MCU, 4:2:0 chroma mean, 8 x 8 orthonormal DCT, quantise /
// dequantise with the sample's two tables, inverse DCT, chroma replication, inverse colour transform, clamp, crop.
//   jpeg_tables_kernel  one workgroup: step count t (read, NOT advanced: the step of sisr_degrade_draw) -> quality [B], tables [B][2][64];
//   jpeg_fwd_kernel     one workgroup per 16 x 64 pixel tile (a whole number of MCUs) and sample: all planes of the tile go through
//                       LDS, three passes over it (columns; rows + quantisation + rows back; columns back).  Nothing intermediate in HBM;
//   jpeg_bwd_kernel     the same tile: every linear stage transposed, the rounding replaced by its surrogate derivative s(u) per
//                       coefficient ('cubic' recomputes u from the saved input in a second set of planes, in double), the replicate pad folded
//                       onto the last row / column.  Gather form, fixed order, no atomics: the same bits on every call.
// The +128 of Cb / Cr and the -128 in front of the DCT cancel and are not executed; luma is carried as Y - 128 between the colour
// transforms.  Quality draw: Philox4x32-10 keyed by the seed, word 3 of the counter DRAW_TAG_QUALITY | rank (sisr_philox.h).  One
// text for host and device (sisr_jpeg_tables_host).  Plain vector stores only.
#include "sisr_dev.h"
#include "sisr_philox.h"

#define JP_TH 16                      // tile: 16 rows x 64 columns = 2 x 8 blocks, 1 x 4 MCUs of 4:2:0
#define JP_TW 64
#define JP_P 65                        // row pitch (floats): 65 mod 32 = 1, see jp_row_pass
#define JP_PLANE (JP_TH * JP_P)
#define JP_TP 9                        // pitch of a table row in LDS: 8 rows on 8 x 9 + k, distinct banks
#define JP_TAB (8 * JP_TP)

// ---- tables -----------------------------------------------------------------------------------------------------------------------
struct JpegDrawArgs {
    uint64_t seed;
    int rank, B, qlo, qhi;
};

// q = min(qlo + (int)((qhi - qlo + 1) u0), qhi) in fp32, u0 = draw_uniform(r0)
__host__ __device__ __forceinline__ int jpeg_draw_quality(const JpegDrawArgs& a, int64_t t, int b) {
    uint32_t r[4];
    draw_words(a.seed, t, (uint32_t)b, DRAW_TAG_QUALITY | (uint32_t)a.rank, r);
    const int q = a.qlo + (int)((float)(a.qhi - a.qlo + 1) * draw_uniform(r[0]));
    return q < a.qhi ? q : a.qhi;
}

// entry i (row-major) of table `tab` (0 luma, 1 chroma) at quality q: libjpeg's integer arithmetic on the Annex K tables
__host__ __device__ __forceinline__ int jpeg_table_entry(int q, int tab, int i) {
    static constexpr unsigned char base[2][64] = {
        {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
         18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
        {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
         99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
    const int s = q < 50 ? 5000 / q : 200 - 2 * q;
    const int v = ((int)base[tab][i] * s + 50) / 100;
    return v < 1 ? 1 : (v > 255 ? 255 : v);
}

static bool jpeg_draw_args_ok(const JpegDrawArgs& a) {
    return a.B >= 1 && a.rank >= 0 && a.rank < DRAW_RANK_LIMIT && a.qlo >= 1 && a.qhi <= 100 && a.qlo <= a.qhi;
}

// One workgroup; the step count is only read (the launch shares the step that sisr_degrade_draw stored in drawn_step)
__global__ void __launch_bounds__(SISR_BLOCK) jpeg_tables_kernel(const int64_t* __restrict__ drawn_step, JpegDrawArgs a,
                                                                  int* __restrict__ quality, float* __restrict__ tables) {
    const int64_t t = *drawn_step;
    for (int it = threadIdx.x; it < a.B * 128; it += SISR_BLOCK) {
        const int b = it >> 7, e = it & 127;
        const int q = jpeg_draw_quality(a, t, b);
        tables[it] = (float)jpeg_table_entry(q, e >> 6, e & 63);
        if (e == 0) quality[b] = q;
    }
}

// ---- the 8-point transform ----------------------------------------------------------------------------------------------------------
// v <- D v (INV: D^T v) with the orthonormal DCT-II matrix D[k][n] = a_k cos((2n + 1) k pi / 16), a_0 = sqrt(1/8), a_k = 1/2: the
// direct product, 8 fused multiply-adds per output in index order.  One text for forward and backward, host and device, and for
// both scalar types (F = double: the surrogate's u in the 'cubic' backward, see jp_row_pass).
template <bool INV, typename F>
__host__ __device__ __forceinline__ void jp_dct8(F (&v)[8]) {
    constexpr F c1 = (F)0.49039264020161522, c2 = (F)0.46193976625564337, c3 = (F)0.41573480615127262, c4 = (F)0.35355339059327376,
                c5 = (F)0.27778511650980111, c6 = (F)0.19134171618254489, c7 = (F)0.09754516100806413;
    constexpr F D[8][8] = {{c4, c4, c4, c4, c4, c4, c4, c4},         {c1, c3, c5, c7, -c7, -c5, -c3, -c1},
                               {c2, c6, -c6, -c2, -c2, -c6, c6, c2},     {c3, -c7, -c1, -c5, c5, c1, c7, -c3},
                               {c4, -c4, -c4, c4, c4, -c4, -c4, c4},     {c5, -c1, c7, c3, -c3, -c7, c1, -c5},
                               {c6, -c2, c2, -c6, -c6, c2, -c2, c6},     {c7, -c5, c3, -c1, c1, -c3, c5, -c7}};
    F o[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        F acc = (F)0;
#pragma unroll
        for (int n = 0; n < 8; ++n) acc = fma(INV ? D[n][k] : D[k][n], v[n], acc);
        o[k] = acc;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = o[k];
}

// ---- the tile in LDS ----------------------------------------------------------------------------------------------------------------
// planes [NPL][16][JP_P]: 0 = Y (- 128), 1, 2 = Cb, Cr at full resolution, 3, 4 = Cb, Cr at half resolution (4:2:0: rows 0..7,
// columns 0..31).  Blocks of the tile in transform order: 4:4:4 16 per plane (b >> 4 = plane), 4:2:0 16 of Y, then 4 + 4 of chroma.
template <int C, bool S420>
struct JpegTile {
    static constexpr int NPL = C == 1 ? 1 : (S420 ? 5 : 3);
    static constexpr int NBLK = S420 ? 24 : 16 * C;
};

// block b -> its plane, origin inside the plane, table; false when the block lies wholly outside the padded image
template <bool S420>
__device__ __forceinline__ bool jp_block(int b, int y0, int x0, int Hp, int Wp, int& plane, int& r0, int& c0, int& tab) {
    if (!S420 || b < 16) {
        plane = b >> 4; r0 = ((b >> 3) & 1) * 8; c0 = (b & 7) * 8; tab = plane ? 1 : 0;
        return y0 + r0 < Hp && x0 + c0 < Wp;
    }
    plane = 3 + ((b - 16) >> 2); r0 = 0; c0 = ((b - 16) & 3) * 8; tab = 1;
    return x0 + 2 * c0 < Wp;
}

// columns of every block: item = (block, column j); consecutive lanes on consecutive floats, 8 reads / writes at the row pitch
template <int NBLK, bool S420, bool INV, typename F>
__device__ __forceinline__ void jp_col_pass(F* __restrict__ pl, int y0, int x0, int Hp, int Wp) {
    for (int it = threadIdx.x; it < NBLK * 8; it += SISR_BLOCK) {
        int plane, r0, c0, tab;
        if (!jp_block<S420>(it >> 3, y0, x0, Hp, Wp, plane, r0, c0, tab)) continue;
        F* p = pl + plane * JP_PLANE + r0 * JP_P + c0 + (it & 7);
        F v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = p[i * JP_P];
        jp_dct8<INV>(v);
#pragma unroll
        for (int i = 0; i < 8; ++i) p[i * JP_P] = v[i];
    }
}

// rows of every block: item = (block, row i) holds row i of the block, then of its coefficients, in registers.  A 32-lane group
// holds rows 0..7 of four neighbouring blocks: float k of the row sits on bank (i + 8 bx + k + const) mod 32 at pitch 65 -- 32
// distinct banks (a double at pitch 65: the two banks 2 (i + 8 bx + k), 64 distinct); the table row on 9 i + k likewise.
//   MODE 0  forward: c = row DCT; c^ = rintf(c / T) T; row DCT back
//   MODE 1  backward 'cubic': u = (row DCT of the image planes pa) / T; g = row DCT of pl; g *= 3 (u - rint u)^2; row DCT back.
//           The image planes and u are DOUBLES: d = u - rint u cancels the integer part of a quotient that fp32 holds to 2^-24 |u|
//           on top of 1e-5 / T from the transforms of pixels near 128, and s = 3 d^2 doubles the relative error: in fp32 dx came
//           out 1.2e-5 .. 3.3e-5 of max |dx| away from float64 autograd at qualities 10 .. 90, in double <= 6.1e-7.
//           s is continuous across a tie, so a u that the forward's fp32 rounded the other way changes nothing.
template <int NBLK, bool S420, int MODE>
__device__ __forceinline__ void jp_row_pass(float* __restrict__ pl, const double* __restrict__ pa, const float* __restrict__ tabs, int y0,
                                            int x0, int Hp, int Wp) {
    for (int it = threadIdx.x; it < NBLK * 8; it += SISR_BLOCK) {
        int plane, r0, c0, tab;
        if (!jp_block<S420>(it >> 3, y0, x0, Hp, Wp, plane, r0, c0, tab)) continue;
        const int i = it & 7, off = plane * JP_PLANE + (r0 + i) * JP_P + c0;
        const float* T = tabs + tab * JP_TAB + i * JP_TP;
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = pl[off + k];
        jp_dct8<false>(v);
        if (MODE == 0) {
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = rintf(v[k] / T[k]) * T[k];
        } else {
            double a[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) a[k] = pa[off + k];
            jp_dct8<false>(a);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const double u = a[k] / (double)T[k], d = u - rint(u);
                v[k] *= (float)(3.0 * d * d);
            }
        }
        jp_dct8<true>(v);
#pragma unroll
        for (int k = 0; k < 8; ++k) pl[off + k] = v[k];
    }
}

// 4:2:0: planes 3, 4 <- scale * (sum of the 2 x 2 pixels of planes 1, 2), added as (a + b) + (c + d)
template <typename F>
__device__ __forceinline__ void jp_chroma_down(F* __restrict__ pl, F scale) {
    for (int it = threadIdx.x; it < 2 * 8 * 32; it += SISR_BLOCK) {
        const int c = it >> 8, rr = (it >> 5) & 7, cc = it & 31;
        const F* s = pl + (1 + c) * JP_PLANE + 2 * rr * JP_P + 2 * cc;
        pl[(3 + c) * JP_PLANE + rr * JP_P + cc] = scale * ((s[0] + s[1]) + (s[JP_P] + s[JP_P + 1]));
    }
}

// four pixels of row `row` (already inside the image) from column gx on, columns clamped to W - 1: one 16-byte load where the
// row is aligned and whole, four 4-byte loads at the ragged end
__device__ __forceinline__ f32x4 jp_load4_clamped(const float* __restrict__ row, int gx, int W, bool vec) {
    if (vec && gx + 3 < W) return *reinterpret_cast<const f32x4*>(row + gx);
    f32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = row[min(gx + j, W - 1)];
    return v;
}
// ... columns >= W read as 0
__device__ __forceinline__ f32x4 jp_load4_zero(const float* __restrict__ row, int gx, int W, bool vec) {
    if (vec && gx + 3 < W) return *reinterpret_cast<const f32x4*>(row + gx);
    f32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = gx + j < W ? row[gx + j] : 0.f;
    return v;
}
__device__ __forceinline__ void jp_store4(float* __restrict__ row, int gx, int W, bool vec, const f32x4 v) {
    if (vec && gx + 3 < W) {
        *reinterpret_cast<f32x4*>(row + gx) = v;
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (gx + j < W) row[gx + j] = v[j];
}

// image -> planes: thread = (row r = tid / 16, four pixels from column 4 (tid % 16) on) of the tile; rows and columns past the
// image replicate its last ones (the pad).  p = (x + 1) 127.5; JFIF YCbCr without the offsets (see the head of the file).
// 16 lanes x 16 bytes: 256 contiguous bytes per row and plane.
template <int C, typename F>
__device__ __forceinline__ void jp_stage_image(const float* __restrict__ img, int H, int W, int y0, int x0, bool vec,
                                               F* __restrict__ pl) {
    const int r = threadIdx.x >> 4, q4 = 4 * (threadIdx.x & 15);
    const int gy = min(y0 + r, H - 1), gx = x0 + q4;
    F ch[C][4];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const f32x4 v = jp_load4_clamped(img + ((int64_t)c * H + gy) * W, gx, W, vec);
#pragma unroll
        for (int j = 0; j < 4; ++j) ch[c][j] = ((F)v[j] + (F)1) * (F)127.5;
    }
    F* d = pl + r * JP_P + q4;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if constexpr (C == 1) {
            d[j] = ch[0][j] - (F)128;
        } else {
            const F R = ch[0][j], G = ch[1][j], B = ch[2][j];
            d[j] = ((F)0.299 * R + (F)0.587 * G + (F)0.114 * B) - (F)128;
            d[JP_PLANE + j] = (F)-0.168735892 * R - (F)0.331264108 * G + (F)0.5 * B;
            d[2 * JP_PLANE + j] = (F)0.5 * R - (F)0.418687589 * G - (F)0.081312411 * B;
        }
    }
}

__device__ __forceinline__ void jp_load_tables(const float* __restrict__ tables, int n, float* __restrict__ tabs) {
    if (threadIdx.x < 128) {
        const int e = threadIdx.x & 63;
        tabs[(threadIdx.x >> 6) * JP_TAB + (e >> 3) * JP_TP + (e & 7)] = tables[(int64_t)n * 128 + threadIdx.x];
    }
}

struct JpegArgs {
    const float *x, *g, *yc, *tables;      // forward: x, tables; backward: g = dy, yc = saved output or NULL, x = saved input ('cubic')
    float* out;
    int H, W, Hp, Wp, clampv, vec;
};

// ---- forward ----------------------------------------------------------------------------------------------------------------------
template <int C, bool S420>
__global__ void __launch_bounds__(SISR_BLOCK) jpeg_fwd_kernel(JpegArgs a) {
    typedef JpegTile<C, S420> TL;
    __shared__ float pl[TL::NPL * JP_PLANE];
    __shared__ float tabs[2 * JP_TAB];
    const int n = blockIdx.z, y0 = blockIdx.y * JP_TH, x0 = blockIdx.x * JP_TW;
    jp_load_tables(a.tables, n, tabs);
    jp_stage_image<C, float>(a.x + (int64_t)n * C * a.H * a.W, a.H, a.W, y0, x0, a.vec, pl);
    __syncthreads();
    if (S420) {
        jp_chroma_down(pl, 0.25f);
        __syncthreads();
    }
    jp_col_pass<TL::NBLK, S420, false, float>(pl, y0, x0, a.Hp, a.Wp);
    __syncthreads();
    jp_row_pass<TL::NBLK, S420, 0>(pl, nullptr, tabs, y0, x0, a.Hp, a.Wp);
    __syncthreads();
    jp_col_pass<TL::NBLK, S420, true, float>(pl, y0, x0, a.Hp, a.Wp);
    __syncthreads();
    // planes -> image: chroma replication, inverse colour transform, clamp, crop, y = p^ / 127.5 - 1
    const int r = threadIdx.x >> 4, q4 = 4 * (threadIdx.x & 15);
    const int gy = y0 + r, gx = x0 + q4;
    if (gy >= a.H || gx >= a.W) return;
    f32x4 o[C];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float Y = pl[r * JP_P + q4 + j] + 128.f;
        float v[3] = {Y, Y, Y};
        if constexpr (C == 3) {
            const int ci = S420 ? 3 * JP_PLANE + (r >> 1) * JP_P + ((q4 + j) >> 1) : JP_PLANE + r * JP_P + q4 + j;
            const float Cb = pl[ci], Cr = pl[ci + JP_PLANE];
            v[0] = Y + 1.402f * Cr;
            v[1] = Y - 0.344136286f * Cb - 0.714136286f * Cr;
            v[2] = Y + 1.772f * Cb;
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float p = a.clampv ? fminf(fmaxf(v[c], 0.f), 255.f) : v[c];
            o[c][j] = p / 127.5f - 1.f;
        }
    }
    float* dst = a.out + (int64_t)n * C * a.H * a.W;
#pragma unroll
    for (int c = 0; c < C; ++c) jp_store4(dst + ((int64_t)c * a.H + gy) * a.W, gx, a.W, a.vec, o[c]);
}

// ---- backward ---------------------------------------------------------------------------------------------------------------------
// g = dy [0 < p^ < 255] / 127.5 inside the image, 0 in the pad; planes <- (M^-1)^T g; 4:2:0: half-resolution chroma <- the sum of
// its 2 x 2 (the transpose of the replication); per coefficient g <- s(u) g between the two transforms (the two table factors
// cancel); the transpose of the chroma mean hands a quarter to each of the 2 x 2; pixel (H - 1, .) collects the padded rows
// H - 1 .. Hp - 1, pixel (., W - 1) the padded columns, rows ascending, columns ascending; dx = 127.5 M^T (...).
// 'ste' (CUBIC = false): s = 1, and D^T D = 1: the transforms are not run at all.
template <int C, bool S420, bool CUBIC>
__global__ void __launch_bounds__(SISR_BLOCK) jpeg_bwd_kernel(JpegArgs a) {
    typedef JpegTile<C, S420> TL;
    __shared__ float pl[TL::NPL * JP_PLANE];
    __shared__ double pa[CUBIC ? TL::NPL * JP_PLANE : 1];          // the image planes of the 'cubic' surrogate, see jp_row_pass
    __shared__ float tabs[CUBIC ? 2 * JP_TAB : 1];
    const int n = blockIdx.z, y0 = blockIdx.y * JP_TH, x0 = blockIdx.x * JP_TW;
    const int r = threadIdx.x >> 4, q4 = 4 * (threadIdx.x & 15);
    const int gy = y0 + r, gx = x0 + q4;
    const int64_t base = (int64_t)n * C * a.H * a.W;
    {
        f32x4 g[C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            g[c] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (gy < a.H && gx < a.W) {
                const int64_t ro = base + ((int64_t)c * a.H + gy) * a.W;
                g[c] = jp_load4_zero(a.g + ro, gx, a.W, a.vec);
                if (a.yc != nullptr) {
                    const f32x4 yv = jp_load4_zero(a.yc + ro, gx, a.W, a.vec);
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (!(yv[j] > -1.f && yv[j] < 1.f)) g[c][j] = 0.f;
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) g[c][j] = g[c][j] / 127.5f;
            }
        }
        float* d = pl + r * JP_P + q4;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if constexpr (C == 1) {
                d[j] = g[0][j];
            } else {
                const float gR = g[0][j], gG = g[1][j], gB = g[2][j];
                d[j] = (gR + gG) + gB;
                d[JP_PLANE + j] = 1.772f * gB - 0.344136286f * gG;
                d[2 * JP_PLANE + j] = 1.402f * gR - 0.714136286f * gG;
            }
        }
    }
    if (CUBIC) {
        jp_load_tables(a.tables, n, tabs);
        jp_stage_image<C, double>(a.x + base, a.H, a.W, y0, x0, a.vec, pa);
    }
    __syncthreads();
    if (S420) {
        jp_chroma_down(pl, 1.f);
        if (CUBIC) jp_chroma_down(pa, 0.25);
        __syncthreads();
    }
    if (CUBIC) {
        jp_col_pass<TL::NBLK, S420, false, float>(pl, y0, x0, a.Hp, a.Wp);
        jp_col_pass<TL::NBLK, S420, false, double>(pa, y0, x0, a.Hp, a.Wp);
        __syncthreads();
        jp_row_pass<TL::NBLK, S420, 1>(pl, pa, tabs, y0, x0, a.Hp, a.Wp);
        __syncthreads();
        jp_col_pass<TL::NBLK, S420, true, float>(pl, y0, x0, a.Hp, a.Wp);
        __syncthreads();
    }
    if (gy >= a.H || gx >= a.W) return;
    f32x4 o[C];
    const int ry1 = gy == a.H - 1 ? a.Hp - 1 : gy;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int px = gx + j;
        float s[3] = {0.f, 0.f, 0.f};
        if (px < a.W) {
            const int rx1 = px == a.W - 1 ? a.Wp - 1 : px;
            for (int ry = gy; ry <= ry1; ++ry) {
                const int ly = ry - y0;
                float row[3] = {0.f, 0.f, 0.f};
                for (int rx = px; rx <= rx1; ++rx) {
                    const int lx = rx - x0;
                    row[0] += pl[ly * JP_P + lx];
                    if constexpr (C == 3) {
                        const int ci = S420 ? 3 * JP_PLANE + (ly >> 1) * JP_P + (lx >> 1) : JP_PLANE + ly * JP_P + lx;
                        row[1] += pl[ci];
                        row[2] += pl[ci + JP_PLANE];
                    }
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) s[c] += row[c];
            }
        }
        if constexpr (C == 1) {
            o[0][j] = s[0] * 127.5f;
        } else {
            const float gY = s[0], gCb = S420 ? 0.25f * s[1] : s[1], gCr = S420 ? 0.25f * s[2] : s[2];
            o[0][j] = (0.299f * gY - 0.168735892f * gCb + 0.5f * gCr) * 127.5f;
            o[1][j] = (0.587f * gY - 0.331264108f * gCb - 0.418687589f * gCr) * 127.5f;
            o[2][j] = (0.114f * gY + 0.5f * gCb - 0.081312411f * gCr) * 127.5f;
        }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) jp_store4(a.out + base + ((int64_t)c * a.H + gy) * a.W, gx, a.W, a.vec, o[c]);
}

// ---- entry points -----------------------------------------------------------------------------------------------------------------
extern "C" int sisr_jpeg_tables(const int64_t* drawn_step_dev, uint64_t seed, int32_t rank, int32_t B, int32_t qlo, int32_t qhi,
                                int32_t* quality_dev, float* tables_dev, void* stream) {
    const JpegDrawArgs a = {seed, rank, B, qlo, qhi};
    if (!drawn_step_dev || !quality_dev || !tables_dev || !jpeg_draw_args_ok(a)) return SISR_E_BADARG;
    if (B > (1 << 23)) return SISR_E_TOOBIG;          // 128 B items are walked with an int
    hipLaunchKernelGGL(jpeg_tables_kernel, dim3(1), dim3(SISR_BLOCK), 0, sisr_stream(stream), drawn_step_dev, a, quality_dev, tables_dev);
    SISR_CHECK_LAUNCH();
    return 0;
}

extern "C" int sisr_jpeg_tables_host(int64_t t, uint64_t seed, int32_t rank, int32_t B, int32_t qlo, int32_t qhi, int32_t* quality_host,
                                     float* tables_host) {
    const JpegDrawArgs a = {seed, rank, B, qlo, qhi};
    if (!quality_host || !tables_host || t < 0 || !jpeg_draw_args_ok(a)) return SISR_E_BADARG;
    for (int b = 0; b < B; ++b) {
        const int q = jpeg_draw_quality(a, t, b);
        quality_host[b] = q;
        for (int e = 0; e < 128; ++e) tables_host[(int64_t)b * 128 + e] = (float)jpeg_table_entry(q, e >> 6, e & 63);
    }
    return 0;
}

// the tile grid of an image, or a status
static int jpeg_plan(int N, int C, int H, int W, int sub, bool s420, const void* p0, const void* p1, const void* p2, JpegArgs& a, dim3& grid) {
    if (N < 1 || H < 1 || W < 1 || (C != 1 && C != 3) || (sub != SISR_JPEG_444 && sub != SISR_JPEG_420)) return SISR_E_BADARG;
    const int mcu = s420 ? 16 : 8;
    const int64_t Hp = ((int64_t)H + mcu - 1) / mcu * mcu, Wp = ((int64_t)W + mcu - 1) / mcu * mcu;
    if (N > 65535 || (Hp + JP_TH - 1) / JP_TH > 65535 || Wp > 0x7FFFFFC0) return SISR_E_TOOBIG;
    a.H = H; a.W = W; a.Hp = (int)Hp; a.Wp = (int)Wp;
    a.vec = W % 4 == 0 && (((uintptr_t)p0 | (uintptr_t)p1 | (uintptr_t)p2) & 15) == 0;
    grid = dim3((unsigned)((Wp + JP_TW - 1) / JP_TW), (unsigned)((Hp + JP_TH - 1) / JP_TH), N);
    return 0;
}

extern "C" int sisr_jpeg_fwd(const float* x, const float* tables, float* y, int32_t N, int32_t C, int32_t H, int32_t W,
                             int32_t subsampling, int32_t clampv, void* stream) {
    if (!x || !tables || !y) return SISR_E_BADARG;
    const bool s420 = subsampling == SISR_JPEG_420 && C == 3;
    JpegArgs a = {x, nullptr, nullptr, tables, y, 0, 0, 0, 0, clampv != 0, 0};
    dim3 grid;
    if (int e = jpeg_plan(N, C, H, W, subsampling, s420, x, y, nullptr, a, grid)) return e;
    hipStream_t st = sisr_stream(stream);
    if (C == 1) hipLaunchKernelGGL((jpeg_fwd_kernel<1, false>), grid, dim3(SISR_BLOCK), 0, st, a);
    else if (s420) hipLaunchKernelGGL((jpeg_fwd_kernel<3, true>), grid, dim3(SISR_BLOCK), 0, st, a);
    else hipLaunchKernelGGL((jpeg_fwd_kernel<3, false>), grid, dim3(SISR_BLOCK), 0, st, a);
    SISR_CHECK_LAUNCH();
    return 0;
}

extern "C" int sisr_jpeg_bwd(const float* dy, const float* y_saved, const float* x_saved, const float* tables, float* dx, int32_t N,
                             int32_t C, int32_t H, int32_t W, int32_t subsampling, int32_t grad, void* stream) {
    if (!dy || !dx || (grad != SISR_JPEG_GRAD_STE && grad != SISR_JPEG_GRAD_CUBIC)) return SISR_E_BADARG;
    const bool cubic = grad == SISR_JPEG_GRAD_CUBIC;
    if (cubic && (!x_saved || !tables)) return SISR_E_BADARG;
    const bool s420 = subsampling == SISR_JPEG_420 && C == 3;
    JpegArgs a = {cubic ? x_saved : nullptr, dy, y_saved, cubic ? tables : nullptr, dx, 0, 0, 0, 0, 0, 0};
    dim3 grid;
    if (int e = jpeg_plan(N, C, H, W, subsampling, s420, dy, dx, (const void*)((uintptr_t)y_saved | (cubic ? (uintptr_t)x_saved : 0)), a, grid)) return e;
    hipStream_t st = sisr_stream(stream);
#define JP_BWD(CC, SS)                                                                                       \
    do {                                                                                                     \
        if (cubic) hipLaunchKernelGGL((jpeg_bwd_kernel<CC, SS, true>), grid, dim3(SISR_BLOCK), 0, st, a);    \
        else hipLaunchKernelGGL((jpeg_bwd_kernel<CC, SS, false>), grid, dim3(SISR_BLOCK), 0, st, a);         \
    } while (0)
    if (C == 1) JP_BWD(1, false);
    else if (s420) JP_BWD(3, true);
    else JP_BWD(3, false);
#undef JP_BWD
    SISR_CHECK_LAUNCH();
    return 0;
}
