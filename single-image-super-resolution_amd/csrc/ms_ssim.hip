// ms_ssim.hip -- multi-scale SSIM (Wang, Simoncelli, Bovik 2003) of two fp32 NCHW batches, forward and backward, entirely on the
// device.  On the view of sisr_ssim.h, applied once at the finest scale, with M = `levels` scales:
//   a_0, b_0 = the view planes;   a_{j+1} = the 2 x 2 mean of a_j, stride 2, no padding (an odd last row / column is dropped)
//   per window position of level j (the window, the "valid" positions and C1, C2 are sisr_ssim.h's):
//       cs = (2 s_ab + C2) / (s_a^2 + s_b^2 + C2),   l = (2 mu_a mu_b + C1) / (mu_a^2 + mu_b^2 + C1)
//   t_j[n,p] = mean over positions of cs (j < M - 1) / of l cs, the SSIM map (j = M - 1)
//   MS[n,p]  = prod_j t_j^{w_j} when every t_j[n,p] > 0, exactly 0 when one of them is <= 0;   ms_ssim[n] = mean_p MS[n,p]
// Nothing here synchronises with the host, nothing uses atomics, every sum has a fixed order: the same bits every call, and the
// launches can sit inside a captured step.
//
// Forward, M + 1 launches: ms_ssim_tile_kernel per level (the tile and LDS scheme of ssim_tile_kernel: 16 x 32 window positions,
// 26 x 42 staged pixels, five row-filtered moments) leaves one (sum of l cs, sum of cs) pair per workgroup and WRITES LEVEL j + 1
// from the pixels it has staged: a workgroup owns its 16 x 32 block, the last tile row / column also the 10 pixels behind it;
// origins and extents are even, so every 2 x 2 cell lies inside exactly one own block.  ms_ssim_finish_kernel folds the partials of
// every (level, plane) of an image in a fixed order in double, writes the terms[M][N][C'] table and the score.
//
// Backward, M launches, coarsest level first, gather form: ms_ssim_bwd_kernel is image_loss_bwd_kernel's scheme (16 x 32 pixel
// tile, 36 x 52 staged pixels, window moments recomputed in LDS, derivative maps filtered by the transposed window) with the map
// S = l cs at the last level and cs = A2 / B2 at the others:
//   d cs/dE_ab = 2 / B2,   d cs/dE_aa = d cs/dE_bb = -cs / B2,   d cs/dmu_a = 2 (cs mu_a - mu_b) / B2   (mu_b: a and b exchanged)
// the factor k_j[n,p] = -g[n] (1 / C') w_j MS[n,p] / t_j[n,p] / (Hv_j Wv_j) formed in the kernel from the terms table (0 when a
// term is <= 0), and the pooling's transpose in the epilogue: pixel (y, x) of level j adds a quarter of grad_{j+1}[y >> 1][x >> 1]
// where that element exists.  Levels >= 1 write their gradient into workspace planes, level 0 writes da / db of the whole image
// (exact zeros in the cropped border, the three channel gradients under luma).  Saved by the forward: the pyramid and the terms.
// LDS: forward 25.4 KB; backward 62,688 B + one float.
#include "sisr_ssim.h"

// every product and sum below is rounded as written (fused multiply-adds are spelled fmaf): the instantiations of the backward
// kernel then compute a gradient with the same instructions, so da is the same bits whether or not db is asked for
#pragma clang fp contract(off)

#define MS_MAX_LEVELS 5
#define MS_BH (SSIM_TH + 2 * SSIM_APRON)      // backward: staged pixels
#define MS_BW (SSIM_TW + 2 * SSIM_APRON)

// what the finish kernel and the backward need of the levels
struct MsLevels {
    int M, planes, N;
    int tiles[MS_MAX_LEVELS];                 // position tiles per (image, plane)
    int part_off[MS_MAX_LEVELS];              // the level's first pair in the partials
    double inv_count[MS_MAX_LEVELS];          // 1 / (Hv_j Wv_j)
    double w[MS_MAX_LEVELS];
};

// one pixel of the view; off: the element of the first plane
__device__ __forceinline__ float ms_load(const float* __restrict__ p, int64_t off, int64_t plane_elems, int luma) {
    return luma ? fmaf(0.114f, p[off + 2 * plane_elems], fmaf(0.587f, p[off + plane_elems], 0.299f * p[off])) : p[off];
}

// workgroup = (image n, plane, tile row, tile column) of level j, flat in that order; part[workgroup][2] = (sum of l cs, sum of cs).
// na / nb (or null at the last level): level j + 1 of a / b, [N][C'][Hn][Wn]
__global__ void __launch_bounds__(SISR_BLOCK) ms_ssim_tile_kernel(const float* __restrict__ a, const float* __restrict__ b, SsimGeom g,
                                                                  SsimWindow win, float c1, float c2, float* __restrict__ part,
                                                                  float* __restrict__ na, float* __restrict__ nb, int Hn, int Wn) {
    constexpr int SH = SSIM_SH, SW = SSIM_SW;
    __shared__ float sa[SH * SW], sb[SH * SW];
    __shared__ float hm[5][SH * SSIM_TW];
    const int tid = threadIdx.x;
    const int tiles = g.tiles_y * g.tiles_x, per_image = g.planes * tiles;
    const int n = blockIdx.x / per_image, r = blockIdx.x - n * per_image;
    const int plane = r / tiles, t = r - plane * tiles;
    const int ty = t / g.tiles_x, tx = t - ty * g.tiles_x;
    const int y0 = ty * SSIM_TH, x0 = tx * SSIM_TW;                   // tile origin in the view
    const int64_t plane_elems = (int64_t)g.H * g.W;
    const int64_t base = ((int64_t)n * g.C + (g.luma ? 0 : plane)) * plane_elems;
    for (int i = tid; i < SH * SW; i += SISR_BLOCK) {
        const int ly = i / SW, lx = i - ly * SW;
        const int y = y0 + ly, x = x0 + lx;
        float va = 0.f, vb = 0.f;
        if (y < g.Hc && x < g.Wc) {
            const int64_t off = base + (int64_t)(y + g.crop) * g.W + (x + g.crop);
            va = ms_load(a, off, plane_elems, g.luma);
            vb = ms_load(b, off, plane_elems, g.luma);
        }
        sa[i] = va;
        sb[i] = vb;
    }
    __syncthreads();
    if (na) {
        // the 2 x 2 cells of this workgroup's own block (even origin, even extent); a cell whose second row / column is outside
        // the level is not written: cell (cy, cx) exists exactly when cy < Hn = Hc >> 1 and cx < Wn = Wc >> 1
        const int own_h = ty == g.tiles_y - 1 ? SH : SSIM_TH, own_w = tx == g.tiles_x - 1 ? SW : SSIM_TW;
        const int ch = own_h >> 1, cw = own_w >> 1;
        const int64_t nbase = ((int64_t)n * g.planes + plane) * Hn * (int64_t)Wn;
        for (int i = tid; i < ch * cw; i += SISR_BLOCK) {
            const int ly = i / cw, lx = i - ly * cw;
            const int cy = (y0 >> 1) + ly, cx = (x0 >> 1) + lx;
            if (cy < Hn && cx < Wn) {
                const int s = (2 * ly) * SW + 2 * lx;
                const int64_t o = nbase + (int64_t)cy * Wn + cx;
                na[o] = 0.25f * ((sa[s] + sa[s + 1]) + (sa[s + SW] + sa[s + SW + 1]));
                nb[o] = 0.25f * ((sb[s] + sb[s + 1]) + (sb[s + SW] + sb[s + SW + 1]));
            }
        }
    }
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
    // vertical pass + the two maps: thread = window column ox, window rows oy and oy + SSIM_TH / 2
    float sums[2] = {0.f, 0.f};                // sum of l cs, sum of cs
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
            const float cs = fmaf(2.f, cov, c2) / (var_a + var_b + c2);
            const float l = fmaf(2.f, mu_ab, c1) / (mu_aa + mu_bb + c1);
            sums[0] += l * cs;
            sums[1] += cs;
        }
    }
    block_partial_sum(sums);
    if (tid == 0) {
        part[2 * (int64_t)blockIdx.x] = sums[0];
        part[2 * (int64_t)blockIdx.x + 1] = sums[1];
    }
}

// prod_j t_j^{w_j} of one (image, plane) from the terms table, in double; `zero`: a term is <= 0 (the score is then exactly 0)
__device__ __forceinline__ double ms_product(const float* terms, const MsLevels& lv, int n, int plane, bool& zero) {
    double m = 1.0;
    zero = false;
    for (int j = 0; j < lv.M; ++j) {
        const float t = terms[((int64_t)j * lv.N + n) * lv.planes + plane];
        if (t <= 0.f) zero = true;
        else m *= pow((double)t, lv.w[j]);
    }
    return m;
}

// one workgroup per image: the partials of every (level, plane) folded in a fixed order in double (fold_partials_double), the
// terms table, the score.  The score is formed from the terms as stored (fp32), so that the backward sees the same product: thread 0
// reads back what it wrote (`terms` is therefore not __restrict__ here)
__global__ void __launch_bounds__(SISR_BLOCK) ms_ssim_finish_kernel(const float* __restrict__ part, MsLevels lv, float* terms,
                                                                    float* __restrict__ ms) {
    const int n = blockIdx.x;
    for (int j = 0; j < lv.M; ++j)
        for (int p = 0; p < lv.planes; ++p) {
            const float* q = part + 2 * ((int64_t)lv.part_off[j] + ((int64_t)n * lv.planes + p) * lv.tiles[j]);
            double s[2];
            fold_partials_double(lv.tiles[j], s, [&](int64_t i, double* acc) { acc[0] += (double)q[2 * i]; acc[1] += (double)q[2 * i + 1]; });
            if (threadIdx.x == 0) terms[((int64_t)j * lv.N + n) * lv.planes + p] = (float)((j == lv.M - 1 ? s[0] : s[1]) * lv.inv_count[j]);
            __syncthreads();                   // the fold's LDS is free again
        }
    if (threadIdx.x == 0) {
        double sum = 0.0;
        for (int p = 0; p < lv.planes; ++p) {
            bool zero;
            const double m = ms_product(terms, lv, n, p, zero);
            sum += zero ? 0.0 : m;
        }
        ms[n] = (float)(sum / (double)lv.planes);
    }
}

// workgroup = (image n, plane, pixel-tile row, pixel-tile column) of the WHOLE level image, flat in that order.  WA / WB: da / db
// wanted.  LAST: the level's map is l cs, else cs.  level: j.  kscale = -(1 / C') / (Hv_j Wv_j).  ua / ub (or null at the coarsest
// level): the gradient planes of level j + 1, [N][C'][Hn][Wn]
template <bool WA, bool WB, bool LAST>
__global__ void __launch_bounds__(SISR_BLOCK) ms_ssim_bwd_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                 const float* __restrict__ terms, const float* __restrict__ gup,
                                                                 SsimGeom g, SsimWindow win, float c1, float c2, MsLevels lv, int level,
                                                                 double kscale, const float* __restrict__ ua,
                                                                 const float* __restrict__ ub, int Hn, int Wn, float* __restrict__ da,
                                                                 float* __restrict__ db) {
    constexpr int NM = 2 + (WA ? 1 : 0) + (WB ? 1 : 0);              // derivative maps: D_q, D_e, D_mua and / or D_mub
    constexpr int MA = 2, MB = WA ? 3 : 2;                           // indices of D_mua / D_mub
    __shared__ float sa[MS_BH * MS_BW], sb[MS_BH * MS_BW];
    __shared__ float hm[5 * MS_BH * SSIM_SW];                          // row-filtered moments [5][MS_BH][SSIM_SW], then maps [NM][SSIM_SH][SSIM_TW]
    __shared__ float dm[4][SSIM_SH * SSIM_SW];
    __shared__ float sk;                                               // k_j[n, plane]
    static_assert(4 * SSIM_SH * SSIM_TW <= 5 * MS_BH * SSIM_SW, "the row-filtered derivative maps reuse the moments' LDS");
    const int tid = threadIdx.x;
    const int tiles = g.btiles_y * g.btiles_x, per_image = g.planes * tiles;
    const int n = blockIdx.x / per_image, r = blockIdx.x - n * per_image;
    const int plane = r / tiles, t = r - plane * tiles;
    const int ty = t / g.btiles_x, tx = t - ty * g.btiles_x;
    const int cy0 = ty * SSIM_TH - g.crop, cx0 = tx * SSIM_TW - g.crop;   // tile origin in the view's coordinates (< 0 in the border)
    const int64_t plane_elems = (int64_t)g.H * g.W;
    const int64_t base = ((int64_t)n * g.C + (g.luma ? 0 : plane)) * plane_elems;
    if (tid == 0) {
        bool zero;
        const double m = ms_product(terms, lv, n, plane, zero);
        const double tj = (double)terms[((int64_t)level * lv.N + n) * lv.planes + plane];
        sk = zero ? 0.f : (float)((double)gup[n] * kscale * lv.w[level] * m / tj);
    }
    // the pixels under every window that touches the tile; outside the view: zeros
    for (int i = tid; i < MS_BH * MS_BW; i += SISR_BLOCK) {
        const int ly = i / MS_BW, lx = i - ly * MS_BW;
        const int y = cy0 - SSIM_APRON + ly, x = cx0 - SSIM_APRON + lx;
        float va = 0.f, vb = 0.f;
        if (y >= 0 && y < g.Hc && x >= 0 && x < g.Wc) {
            const int64_t off = base + (int64_t)(y + g.crop) * g.W + (x + g.crop);
            va = ms_load(a, off, plane_elems, g.luma);
            vb = ms_load(b, off, plane_elems, g.luma);
        }
        sa[i] = va;
        sb[i] = vb;
    }
    __syncthreads();
    const float ksn = sk;
    // horizontal pass: every staged row at the SSIM_SW position columns (lanes on consecutive columns)
    for (int i = tid; i < MS_BH * SSIM_SW; i += SISR_BLOCK) {
        const int ly = i / SSIM_SW, ox = i - ly * SSIM_SW;
        const float* pa = sa + ly * MS_BW + ox;
        const float* pb = sb + ly * MS_BW + ox;
        float ma = 0.f, mb = 0.f, maa = 0.f, mbb = 0.f, mab = 0.f;
#pragma unroll
        for (int k = 0; k < SSIM_WIN; ++k) {
            const float w = win.w[k], u = pa[k], v = pb[k];
            const float wu = w * u, wv = w * v;
            ma += wu; mb += wv;
            maa = fmaf(wu, u, maa); mbb = fmaf(wv, v, mbb); mab = fmaf(wu, v, mab);
        }
        hm[i] = ma; hm[MS_BH * SSIM_SW + i] = mb; hm[2 * (MS_BH * SSIM_SW) + i] = maa;
        hm[3 * (MS_BH * SSIM_SW) + i] = mbb; hm[4 * (MS_BH * SSIM_SW) + i] = mab;
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
            for (int q = 0; q < 5; ++q) m[q] = fmaf(w, hm[q * (MS_BH * SSIM_SW) + i + k * SSIM_SW], m[q]);
        }
        const int py = cy0 - SSIM_APRON + qy, px = cx0 - SSIM_APRON + qx;
        const bool valid = py >= 0 && py < g.Hv && px >= 0 && px < g.Wv;
        const float mu_aa = m[0] * m[0], mu_bb = m[1] * m[1], mu_ab = m[0] * m[1];
        const float a2 = fmaf(2.f, m[4] - mu_ab, c2);
        const float rb2 = 1.f / ((m[2] - mu_aa) + (m[3] - mu_bb) + c2);
        if constexpr (LAST) {
            const float a1 = fmaf(2.f, mu_ab, c1);
            const float rb1 = 1.f / (mu_aa + mu_bb + c1);
            const float r12 = rb1 * rb2;
            const float s = a1 * a2 * r12;
            const float cross = 2.f * (a2 - a1) * r12, self = 2.f * s * (rb2 - rb1);
            dm[0][i] = valid ? -s * rb2 : 0.f;
            dm[1][i] = valid ? 2.f * a1 * r12 : 0.f;
            if (WA) dm[MA][i] = valid ? fmaf(m[1], cross, m[0] * self) : 0.f;
            if (WB) dm[MB][i] = valid ? fmaf(m[0], cross, m[1] * self) : 0.f;
        } else {
            const float cs = a2 * rb2;
            dm[0][i] = valid ? -cs * rb2 : 0.f;
            dm[1][i] = valid ? 2.f * rb2 : 0.f;
            if (WA) dm[MA][i] = valid ? 2.f * fmaf(cs, m[0], -m[1]) * rb2 : 0.f;
            if (WB) dm[MB][i] = valid ? 2.f * fmaf(cs, m[1], -m[0]) * rb2 : 0.f;
        }
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
    // vertical + the pooling's transpose + store: thread = pixel column px, pixel rows py and py + SSIM_TH / 2
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
            float tq[NM];
#pragma unroll
            for (int q = 0; q < NM; ++q) tq[q] = 0.f;
#pragma unroll
            for (int k = 0; k < SSIM_WIN; ++k) {
                const float w = win.w[k];
#pragma unroll
                for (int q = 0; q < NM; ++q) tq[q] = fmaf(w, hm[q * (SSIM_SH * SSIM_TW) + (py + k) * SSIM_TW + px], tq[q]);
            }
            const float va = sa[(py + SSIM_APRON) * MS_BW + px + SSIM_APRON];
            const float vb = sb[(py + SSIM_APRON) * MS_BW + px + SSIM_APRON];
            if (ksn != 0.f) {                                         // k = 0: exact zeros, whatever the maps hold
                if (WA) ga = ksn * fmaf(vb, tq[1], fmaf(2.f * va, tq[0], tq[MA]));
                if (WB) gb = ksn * fmaf(va, tq[1], fmaf(2.f * vb, tq[0], tq[MB]));
            }
            if (ua != nullptr && (y >> 1) < Hn && (x >> 1) < Wn) {
                const int64_t uo = (((int64_t)n * g.planes + plane) * Hn + (y >> 1)) * (int64_t)Wn + (x >> 1);
                if (WA) ga = fmaf(0.25f, ua[uo], ga);
                if (WB) gb = fmaf(0.25f, ub[uo], gb);
            }
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

// ---- host ------------------------------------------------------------------------------------------------------------------------
struct MsPlan {
    int M;
    SsimGeom g[MS_MAX_LEVELS];                // level 0: the view of the inputs; levels >= 1: plain [N][C'][H_j][W_j]
    int64_t pyr_off[MS_MAX_LEVELS];           // the level's first float in a pyramid buffer (levels >= 1)
    int64_t pyr_floats, part_floats;
    MsLevels lv;
};

// 0, or the status code of the shapes
static int ms_plan(int N, int C, int H, int W, int crop, int luma, int levels, MsPlan& p) {
    if (N <= 0) return SISR_E_BADARG;
    if (C != 1 && C != 3) return SISR_E_UNSUPPORTED;
    if (levels < 1 || levels > MS_MAX_LEVELS) return SISR_E_BADARG;
    if (!ssim_geom(C, H, W, crop, luma, SSIM_APRON, p.g[0])) return SISR_E_BADARG;
    p.M = levels;
    const int planes = p.g[0].planes;
    for (int j = 1; j < levels; ++j) {
        const int hj = p.g[0].Hc >> j, wj = p.g[0].Wc >> j;
        if (!ssim_geom(planes, hj, wj, 0, 0, SSIM_APRON, p.g[j])) return SISR_E_BADARG;      // a level below 11 pixels
    }
    p.lv.M = levels; p.lv.planes = planes; p.lv.N = N;
    int64_t pyr = 0, pairs = 0;
    for (int j = 0; j < levels; ++j) {
        const SsimGeom& g = p.g[j];
        p.pyr_off[j] = pyr;
        if (j > 0) pyr += (int64_t)N * planes * g.H * g.W;
        if (pairs > INT32_MAX) return SISR_E_TOOBIG;
        p.lv.part_off[j] = (int)pairs;
        p.lv.tiles[j] = g.tiles_y * g.tiles_x;
        p.lv.inv_count[j] = 1.0 / ((double)g.Hv * g.Wv);
        p.lv.w[j] = 0.0;
        pairs += (int64_t)N * planes * g.tiles_y * g.tiles_x;
        if ((int64_t)N * planes * g.btiles_y * g.btiles_x > INT32_MAX) return SISR_E_TOOBIG;   // the backward's grid
    }
    for (int j = levels; j < MS_MAX_LEVELS; ++j) { p.lv.part_off[j] = 0; p.lv.tiles[j] = 0; p.lv.inv_count[j] = 0.0; p.lv.w[j] = 0.0; }
    p.pyr_floats = pyr;
    p.part_floats = 2 * pairs;
    if (p.part_floats > INT32_MAX || 2 * pyr > INT32_MAX) return SISR_E_TOOBIG;
    return 0;
}

// data_range and the first `levels` weights: positive and finite (a NaN fails the comparison)
static bool ms_scalars_ok(float data_range, int levels, const float* weights) {
    if (!weights || !(data_range > 0.f) || !std::isfinite(data_range)) return false;
    for (int j = 0; j < levels; ++j)
        if (!(weights[j] > 0.f) || !std::isfinite(weights[j])) return false;
    return true;
}

extern "C" int sisr_ms_ssim_ws_floats(int32_t N, int32_t C, int32_t H, int32_t W, int32_t crop, int32_t luma, int32_t levels,
                                      int32_t which) {
    MsPlan p;
    const int e = ms_plan(N, C, H, W, crop, luma, levels, p);
    if (e) return e;
    if (which == 0) return (int)p.pyr_floats;
    if (which == 1) return (int)p.part_floats;
    if (which == 2) return (int)(2 * p.pyr_floats);
    return SISR_E_BADARG;
}

extern "C" int sisr_ms_ssim_fwd(const float* a, const float* b, int32_t N, int32_t C, int32_t H, int32_t W, int32_t crop, int32_t luma,
                                float data_range, int32_t levels, const float* weights, float* pyr_a, float* pyr_b, float* part,
                                float* terms, float* ms, void* stream) {
    MsPlan p;
    const int e = ms_plan(N, C, H, W, crop, luma, levels, p);
    if (e) return e;
    if (!a || !b || !part || !terms || !ms || (levels > 1 && (!pyr_a || !pyr_b)) || !ms_scalars_ok(data_range, levels, weights))
        return SISR_E_BADARG;
    for (int j = 0; j < levels; ++j) p.lv.w[j] = (double)weights[j];
    const double L = (double)data_range;
    const float c1 = (float)(0.01 * L * 0.01 * L), c2 = (float)(0.03 * L * 0.03 * L);
    const SsimWindow win = ssim_window();
    hipStream_t st = sisr_stream(stream);
    for (int j = 0; j < levels; ++j) {
        const SsimGeom& g = p.g[j];
        const float* aj = j == 0 ? a : pyr_a + p.pyr_off[j];
        const float* bj = j == 0 ? b : pyr_b + p.pyr_off[j];
        const bool pool = j + 1 < levels;
        float* na = pool ? pyr_a + p.pyr_off[j + 1] : nullptr;
        float* nb = pool ? pyr_b + p.pyr_off[j + 1] : nullptr;
        const int Hn = pool ? p.g[j + 1].H : 0, Wn = pool ? p.g[j + 1].W : 0;
        hipLaunchKernelGGL(ms_ssim_tile_kernel, dim3((unsigned)((int64_t)N * g.planes * p.lv.tiles[j])), dim3(SISR_BLOCK), 0, st, aj, bj,
                           g, win, c1, c2, part + 2 * (int64_t)p.lv.part_off[j], na, nb, Hn, Wn);
        SISR_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(ms_ssim_finish_kernel, dim3((unsigned)N), dim3(SISR_BLOCK), 0, st, (const float*)part, p.lv, terms, ms);
    SISR_CHECK_LAUNCH();
    return 0;
}

template <bool WA, bool WB>
static void ms_bwd_launch(bool last, unsigned wgs, hipStream_t st, const float* a, const float* b, const float* terms, const float* gup,
                          const SsimGeom& g, const SsimWindow& win, float c1, float c2, const MsLevels& lv, int level, double kscale,
                          const float* ua, const float* ub, int Hn, int Wn, float* da, float* db) {
    if (last)
        hipLaunchKernelGGL((ms_ssim_bwd_kernel<WA, WB, true>), dim3(wgs), dim3(SISR_BLOCK), 0, st, a, b, terms, gup, g, win, c1, c2, lv,
                           level, kscale, ua, ub, Hn, Wn, da, db);
    else
        hipLaunchKernelGGL((ms_ssim_bwd_kernel<WA, WB, false>), dim3(wgs), dim3(SISR_BLOCK), 0, st, a, b, terms, gup, g, win, c1, c2, lv,
                           level, kscale, ua, ub, Hn, Wn, da, db);
}

extern "C" int sisr_ms_ssim_bwd(const float* a, const float* b, const float* pyr_a, const float* pyr_b, const float* terms,
                                const float* gup, int32_t N, int32_t C, int32_t H, int32_t W, int32_t crop, int32_t luma,
                                float data_range, int32_t levels, const float* weights, float* work, float* da, float* db,
                                void* stream) {
    MsPlan p;
    const int e = ms_plan(N, C, H, W, crop, luma, levels, p);
    if (e) return e;
    if (!a || !b || !terms || !gup || (!da && !db) || (levels > 1 && (!pyr_a || !pyr_b || !work)) ||
        !ms_scalars_ok(data_range, levels, weights))
        return SISR_E_BADARG;
    for (int j = 0; j < levels; ++j) p.lv.w[j] = (double)weights[j];
    const double L = (double)data_range;
    const float c1 = (float)(0.01 * L * 0.01 * L), c2 = (float)(0.03 * L * 0.03 * L);
    const SsimWindow win = ssim_window();
    hipStream_t st = sisr_stream(stream);
    // work: the gradient planes of levels >= 1, a's then b's, each laid out as a pyramid buffer
    float* wa = work;
    float* wb = work ? work + p.pyr_floats : nullptr;
    for (int j = levels - 1; j >= 0; --j) {
        const SsimGeom& g = p.g[j];
        const float* aj = j == 0 ? a : pyr_a + p.pyr_off[j];
        const float* bj = j == 0 ? b : pyr_b + p.pyr_off[j];
        const bool up = j + 1 < levels;
        const float* ua = up ? wa + p.pyr_off[j + 1] : nullptr;
        const float* ub = up ? wb + p.pyr_off[j + 1] : nullptr;
        const int Hn = up ? p.g[j + 1].H : 0, Wn = up ? p.g[j + 1].W : 0;
        float* oa = j == 0 ? da : (da ? wa + p.pyr_off[j] : nullptr);
        float* ob = j == 0 ? db : (db ? wb + p.pyr_off[j] : nullptr);
        const double kscale = -(1.0 / (double)g.planes) * p.lv.inv_count[j];
        const unsigned wgs = (unsigned)((int64_t)N * g.planes * g.btiles_y * g.btiles_x);
        const bool last = j == levels - 1;
        if (da && db) ms_bwd_launch<true, true>(last, wgs, st, aj, bj, terms, gup, g, win, c1, c2, p.lv, j, kscale, ua, ub, Hn, Wn, oa, ob);
        else if (da) ms_bwd_launch<true, false>(last, wgs, st, aj, bj, terms, gup, g, win, c1, c2, p.lv, j, kscale, ua, ub, Hn, Wn, oa, ob);
        else ms_bwd_launch<false, true>(last, wgs, st, aj, bj, terms, gup, g, win, c1, c2, p.lv, j, kscale, ua, ub, Hn, Wn, oa, ob);
        SISR_CHECK_LAUNCH();
    }
    return 0;
}
