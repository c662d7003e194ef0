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
// Forward, M + 1 launches: ms_ssim_tile_kernel per level (the tile and LDS scheme of ssim_tile_kernel, compiled here with
// contraction off: 16 x 32 window positions, 26 x 42 staged pixels, five row-filtered moments) leaves one (sum of l cs, sum of cs) pair per
// workgroup and WRITES LEVEL j + 1 from the pixels it has staged: a workgroup owns its 16 x 32 block, the last tile row / column
// also the 10 pixels behind it; origins and extents are even, so every 2 x 2 cell lies inside exactly one own block.
// ms_ssim_finish_kernel folds the partials of every (level, plane) of an image in a fixed order in double, writes the
// terms[M][N][C'] table and the score.
//
// Backward, M launches, coarsest level first: ms_ssim_bwd_kernel runs the tile scheme of sisr_ssim_bwd.h with the map l cs at the
// last level and cs at the others, multiplies the window gradient by the factor k_j[n,p] = -g[n] (1 / C') w_j MS[n,p] / t_j[n,p] /
// (Hv_j Wv_j), formed in the kernel from the terms table (0 when a term is <= 0), and adds the pooling's transpose: pixel (y, x)
// of level j adds a quarter of grad_{j+1}[y >> 1][x >> 1] where that element exists.  Levels >= 1 write their gradient into
// workspace planes, level 0 writes da / db of the whole image (exact zeros in the cropped border, the three channel gradients
// under luma).  Saved by the forward: the pyramid and the terms.
// LDS: forward 25.4 KB; backward 62,688 B + one float.

// contraction is off from this include to the end of the file (the include-order rule is written down in this header)
#include "sisr_ssim_bwd.h"

#define MS_MAX_LEVELS 5

// what the finish kernel and the backward need of the levels
struct MsLevels {
    int M, planes, N;
    int tiles[MS_MAX_LEVELS];                 // position tiles per (image, plane)
    int part_off[MS_MAX_LEVELS];              // the level's first pair in the partials
    double inv_count[MS_MAX_LEVELS];          // 1 / (Hv_j Wv_j)
    double w[MS_MAX_LEVELS];
};

// workgroup = (image n, plane, tile row, tile column) of level j, flat in that order; part[workgroup][2] = (sum of l cs, sum of cs).
// na / nb (or null at the last level): level j + 1 of a / b, [N][C'][Hn][Wn]
__global__ void __launch_bounds__(SISR_BLOCK) ms_ssim_tile_kernel(const float* __restrict__ a, const float* __restrict__ b, SsimGeom g,
                                                                  SsimWindow win, float c1, float c2, float* __restrict__ part,
                                                                  float* __restrict__ na, float* __restrict__ nb, int Hn, int Wn) {
    constexpr int SH = SSIM_SH, SW = SSIM_SW;
    __shared__ float sa[SH * SW], sb[SH * SW];
    __shared__ float hm[5][SH * SSIM_TW];
    const int tid = threadIdx.x;
    const SsimTile t = ssim_tile(g, g.tiles_y, g.tiles_x);
    const int y0 = t.ty * SSIM_TH, x0 = t.tx * SSIM_TW;               // tile origin in the view
    for (int i = tid; i < SH * SW; i += SISR_BLOCK) {
        const int ly = i / SW, lx = i - ly * SW;
        const int y = y0 + ly, x = x0 + lx;
        float va = 0.f, vb = 0.f;
        if (y < g.Hc && x < g.Wc) {
            const int64_t off = t.base + (int64_t)(y + g.crop) * g.W + (x + g.crop);
            va = ssim_view_load(a, off, t.plane_elems, g.luma);
            vb = ssim_view_load(b, off, t.plane_elems, g.luma);
        }
        sa[i] = va;
        sb[i] = vb;
    }
    __syncthreads();
    if (na) {
        // the 2 x 2 cells of this workgroup's own block (even origin, even extent); a cell whose second row / column is outside
        // the level is not written: cell (cy, cx) exists exactly when cy < Hn = Hc >> 1 and cx < Wn = Wc >> 1
        const int own_h = t.ty == g.tiles_y - 1 ? SH : SSIM_TH, own_w = t.tx == g.tiles_x - 1 ? SW : SSIM_TW;
        const int ch = own_h >> 1, cw = own_w >> 1;
        const int64_t nbase = ((int64_t)t.n * g.planes + t.plane) * Hn * (int64_t)Wn;
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

// the workgroups of ssim_bwd_tile over the WHOLE level image.  WA / WB: da / db wanted.  LAST: the level's map is l cs, else cs.
// level: j.  kscale = -(1 / C') / (Hv_j Wv_j).  ua / ub (or null at the coarsest level): the gradient planes of level j + 1,
// [N][C'][Hn][Wn]
template <bool WA, bool WB, bool LAST>
__global__ void __launch_bounds__(SISR_BLOCK) ms_ssim_bwd_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                 const float* __restrict__ terms, const float* __restrict__ gup,
                                                                 SsimGeom g, SsimWindow win, float c1, float c2, MsLevels lv, int level,
                                                                 double kscale, const float* __restrict__ ua,
                                                                 const float* __restrict__ ub, int Hn, int Wn, float* __restrict__ da,
                                                                 float* __restrict__ db) {
    __shared__ SsimBwdLds lds;
    __shared__ float sk;                                               // k_j[n, plane]
    const SsimBwdTile t = ssim_bwd_tile(g);
    if (threadIdx.x == 0) {
        bool zero;
        const double m = ms_product(terms, lv, t.n, t.plane, zero);
        const double tj = (double)terms[((int64_t)level * lv.N + t.n) * lv.planes + t.plane];
        sk = zero ? 0.f : (float)((double)gup[t.n] * kscale * lv.w[level] * m / tj);
    }
    ssim_bwd_filter_maps<WA, WB, LAST ? SSIM_MAP_LCS : SSIM_MAP_CS>(a, b, g, win, c1, c2, t, lds);
    const float ksn = sk;                                              // behind the barriers of the phases above
    ssim_bwd_pixels<WA, WB>(g, t, da, db, [&](int py, int px, int y, int x, int64_t, float& ga, float& gb) {
        float va, vb, wa, wb;
        ssim_bwd_window_grad<WA, WB>(win, lds, py, px, va, vb, wa, wb);
        if (ksn != 0.f) {                                             // k = 0: exact zeros, whatever the maps hold
            if (WA) ga = ksn * wa;
            if (WB) gb = ksn * wb;
        }
        // the pooling's transpose
        if (ua != nullptr && (y >> 1) < Hn && (x >> 1) < Wn) {
            const int64_t uo = (((int64_t)t.n * g.planes + t.plane) * Hn + (y >> 1)) * (int64_t)Wn + (x >> 1);
            if (WA) ga = fmaf(0.25f, ua[uo], ga);
            if (WB) gb = fmaf(0.25f, ub[uo], gb);
        }
    });
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
    float c1, c2;
    ssim_constants((double)data_range, c1, c2);
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
    float c1, c2;
    ssim_constants((double)data_range, c1, c2);
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
        ssim_bwd_dispatch(da, db, [&](auto wa, auto wb) {
            constexpr bool WA = decltype(wa)::value, WB = decltype(wb)::value;
            auto* kernel = j == levels - 1 ? ms_ssim_bwd_kernel<WA, WB, true> : ms_ssim_bwd_kernel<WA, WB, false>;
            hipLaunchKernelGGL(kernel, dim3(wgs), dim3(SISR_BLOCK), 0, st, aj, bj, terms, gup, g, win, c1, c2, p.lv, j, kscale, ua, ub,
                               Hn, Wn, oa, ob);
        });
        SISR_CHECK_LAUNCH();
    }
    return 0;
}
