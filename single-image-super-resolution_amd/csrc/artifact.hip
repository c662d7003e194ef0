// artifact.hip -- the artifact-aware (locally discriminative, LDL) loss of Liang et al., "Details or Artifacts" (CVPR 2022): the refined
// artifact map and the L1 it weighs, forward and backward.  sr, gt, ema: fp32 [N][C][H][W], C 1 or 3; K odd,
// 3 .. SISR_ARTIFACT_MAX_K, P = K / 2, H > P, W > P:
//   r_sr = sum_c |gt - sr|,  r_ema = sum_c |gt - ema|                                  [N][H][W]
//   p[n] = Var(r_sr[n])^(1/5)  (divisor H W - 1)
//   v    = Var of r_sr[n] over the K x K window (divisor K K - 1), the border mirrored as in gauss.hip: -q below 0, 2 (L - 1) - q from L on
//   map  = p v, exactly 0 where r_sr < r_ema (strict);   loss[n] = weight sum_{y,x} map r_sr / (C H W)
//   the map is a constant of the loss:  dsr = g[n] weight map sign(sr - gt) / (C H W),  dgt = -dsr
// Forward, three launches (two for the map alone):
//   artifact_residual_kernel  reads the three images once, writes the two residual planes, and leaves one (count, mean, M2) partial
//                             of r_sr per workgroup: sums of r - r0 and (r - r0)^2 in double around the workgroup's first value r0
//   artifact_tile_kernel      a workgroup owns an AT_TH x AT_TW tile of one sample: merges the sample's partials (shifted sums in double,
//                             fixed order: every workgroup of a sample gets the same p[n]), stages the r_sr tile with a halo of P into
//                             LDS (the border resolved while staging; every global load of the workgroup is in flight before the first
//                             is waited for), takes the window variance in two passes (mean, then squared deviations; a thread owns
//                             two pixels of one column; K is a template parameter, so the window loops unroll), masks,
//                             stores the map and leaves the tile's sum of map r_sr (|sr - gt| summed over c IS r_sr: sr is not read again)
//   artifact_finish_kernel    per sample a fixed-order sum of the tile partials in double
// Backward: one elementwise launch.  No atomics, plain vector stores, nothing read back by the host: the same bits on every call.
#include "sisr_dev.h"

#include <cmath>

#define AT_TH 8
#define AT_TW 64
#define AT_PMAX (SISR_ARTIFACT_MAX_K / 2)
#define AT_SW (AT_TW + 2 * AT_PMAX)               // pitch of the staged tile
#define AT_SH (AT_TH + 2 * AT_PMAX)
#define AT_PX (AT_TH / (SISR_BLOCK / 64))         // pixels of a thread: consecutive rows of one column
#define AT_MAX_PARTS SISR_BLOCK                   // variance partials of a sample: one term per thread of the merge in the tile kernel
static_assert(AT_TW == 64 && SISR_BLOCK == 256, "a wave's lanes are the tile's columns; four waves share the rows");
static_assert(AT_PX == 2 && SISR_ARTIFACT_MAX_K == 11, "the row loop is split at AT_PX - 1 and K; K >= 3 > AT_PX - 1");

// the workspace: doubles first (8-byte aligned), then the planes
struct ArtifactWs {
    double* stats;        // [N][parts][3]: count, mean, M2 of r_sr over the workgroup's pixels
    double* tile_sum;     // [N][tiles]: sum of map r_sr over the tile
    float* r_sr;          // [N][H][W]
    float* r_ema;         // [N][H][W]
    int parts, chunk;     // workgroups of a sample in the first launch, quads (4 pixels) of each
    int tiles_x, tiles_y;
    int64_t floats;
};

// -> 0 or a status code.  ws may be NULL (the size query)
static int artifact_ws(int64_t N, int64_t H, int64_t W, void* ws, ArtifactWs& a) {
    if (N < 1 || H < 1 || W < 1) return SISR_E_BADARG;
    if (H * W > INT32_MAX || N > INT32_MAX / (H * W)) return SISR_E_TOOBIG;
    const int64_t hw = H * W, quads = (hw + 3) / 4;
    int64_t parts = (quads + SISR_BLOCK - 1) / SISR_BLOCK;
    if (parts > AT_MAX_PARTS) parts = AT_MAX_PARTS;
    a.chunk = (int)((quads + parts - 1) / parts);
    a.parts = (int)((quads + a.chunk - 1) / a.chunk);             // no workgroup without a pixel
    a.tiles_y = (int)((H + AT_TH - 1) / AT_TH);
    a.tiles_x = (int)((W + AT_TW - 1) / AT_TW);
    const int64_t tiles = (int64_t)a.tiles_y * a.tiles_x;
    const int64_t doubles = (N * (3 * a.parts + tiles) + 1) & ~(int64_t)1;      // even: the planes start on a 16-byte line of ws
    a.floats = 2 * doubles + 2 * N * hw;
    if (a.floats > INT32_MAX) return SISR_E_TOOBIG;
    a.stats = (double*)ws;
    a.tile_sum = a.stats + N * 3 * a.parts;
    a.r_sr = (float*)ws + 2 * doubles;
    a.r_ema = a.r_sr + N * hw;
    return 0;
}

// four consecutive elements from p + off; VEC: one 16-byte access, else `valid` scalar ones
template <bool VEC>
__device__ __forceinline__ f32x4 at_load4(const float* __restrict__ p, int64_t off, int valid) {
    if (VEC) return *reinterpret_cast<const f32x4*>(p + off);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (j < valid) v[j] = p[off + j];
    return v;
}
template <bool VEC>
__device__ __forceinline__ void at_store4(float* __restrict__ p, int64_t off, int valid, const f32x4 v) {
    if (VEC) {
        *reinterpret_cast<f32x4*>(p + off) = v;
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (j < valid) p[off + j] = v[j];
}

// ---- launch 1: blockIdx.x = n * parts + part ------------------------------------------------------------------------------------
template <int C, bool VEC>
__global__ void __launch_bounds__(SISR_BLOCK) artifact_residual_kernel(const float* __restrict__ sr, const float* __restrict__ gt,
                                                                       const float* __restrict__ ema, int hw, ArtifactWs a) {
    const int n = blockIdx.x / a.parts, part = blockIdx.x - n * a.parts;
    const int quads = (hw + 3) >> 2;
    const int q0 = part * a.chunk, q1 = min(q0 + a.chunk, quads);
    const int64_t img = (int64_t)n * C * hw, plane = (int64_t)n * hw;
    // the shift of this workgroup's sums: its first residual
    float r0 = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) r0 += fabsf(gt[img + (int64_t)c * hw + 4 * q0] - sr[img + (int64_t)c * hw + 4 * q0]);
    double s[2] = {0.0, 0.0};
    for (int q = q0 + (int)threadIdx.x; q < q1; q += SISR_BLOCK) {
        const int valid = min(4, hw - 4 * q);
        f32x4 rs = {0.f, 0.f, 0.f, 0.f}, re = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const int64_t off = img + (int64_t)c * hw + 4 * q;
            const f32x4 g = at_load4<VEC>(gt, off, valid), x = at_load4<VEC>(sr, off, valid), e = at_load4<VEC>(ema, off, valid);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                rs[j] += fabsf(g[j] - x[j]);
                re[j] += fabsf(g[j] - e[j]);
            }
        }
        at_store4<VEC>(a.r_sr, plane + 4 * q, valid, rs);
        at_store4<VEC>(a.r_ema, plane + 4 * q, valid, re);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < valid) {
                const double d = (double)rs[j] - (double)r0;
                s[0] += d;
                s[1] = fma(d, d, s[1]);
            }
    }
    block_partial_sum<double, 2>(s);
    if (threadIdx.x == 0) {
        const double cnt = (double)(min(4 * q1, hw) - 4 * q0);
        const double m2 = s[1] - s[0] * s[0] / cnt;
        double* o = a.stats + ((int64_t)n * a.parts + part) * 3;
        o[0] = cnt;
        o[1] = (double)r0 + s[0] / cnt;
        o[2] = m2 < 0.0 ? 0.0 : m2;                        // (a NaN stays a NaN)
    }
}

// the pixel a padded coordinate reads; coordinates farther out than the mirror reaches (rows and columns of a ragged tile that no
// stored pixel reads) are clamped onto the plane so that every staged value is a value of the plane
__device__ __forceinline__ int at_mirror(int q, int L) {
    q = q < 0 ? -q : (q >= L ? 2 * (L - 1) - q : q);
    return min(max(q, 0), L - 1);
}

// One pass over the K x K windows of a thread's AT_PX pixels (consecutive rows of one column): staged rows j .. j + K - 1 of columns
// 0 .. K - 1 from src.  Row i of the K + AT_PX - 1 rows belongs to pixel j for 0 <= i - j < K, so a staged value is read once for the
// AT_PX pixels; K is a compile-time constant: the loops unroll and a column's LDS reads are in flight together.  A column's K terms are
// added in fp32, the K columns in double.  SECOND: the terms are (value - mean[j])^2, else the values
template <int K, bool SECOND>
__device__ __forceinline__ void at_window(const float* src0, const float (&mean)[AT_PX], double (&out)[AT_PX]) {
#pragma unroll
    for (int j = 0; j < AT_PX; ++j) out[j] = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        float v[K + AT_PX - 1], cs[AT_PX];
#pragma unroll
        for (int i = 0; i < K + AT_PX - 1; ++i) v[i] = src0[i * AT_SW + k];
#pragma unroll
        for (int j = 0; j < AT_PX; ++j) {
            cs[j] = 0.f;
#pragma unroll
            for (int i = j; i < j + K; ++i) {
                if (SECOND) {
                    const float d = v[i] - mean[j];
                    cs[j] = fmaf(d, d, cs[j]);
                } else {
                    cs[j] += v[i];
                }
            }
            out[j] += (double)cs[j];
        }
    }
}

// ---- launch 2: blockIdx.x = n * tiles + tile ------------------------------------------------------------------------------------
template <int K>
__global__ void __launch_bounds__(SISR_BLOCK) artifact_tile_kernel(ArtifactWs a, int H, int W, float* __restrict__ map, int with_loss) {
    constexpr int P = K / 2, SH = AT_TH + 2 * P, SC = AT_TW + 2 * P;      // the staged rows and columns (SC <= 74: two loads per lane)
    constexpr int SROWS = (SH + SISR_BLOCK / 64 - 1) / (SISR_BLOCK / 64);  // staged rows of a wave
    __shared__ float tile[AT_SH * AT_SW];
    __shared__ double patch_weight;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tiles = a.tiles_x * a.tiles_y;
    const int n = blockIdx.x / tiles, t = blockIdx.x - n * tiles;
    const int ty = t / a.tiles_x, tx = t - ty * a.tiles_x;
    const int y0 = ty * AT_TH, x0 = tx * AT_TW;
    const int r0 = wave * AT_PX;
    const int64_t plane = (int64_t)n * H * W;
    const float* __restrict__ rsr = a.r_sr + plane;

    // ---- every global load of the workgroup is issued before the first one is waited for: r_ema of this thread's pixels, its share
    // of the tile (a wave per row, rows wave, wave + 4, ...), its term of the patch weight
    float re[AT_PX], sv[SROWS][2];
#pragma unroll
    for (int j = 0; j < AT_PX; ++j) {
        const int y = y0 + r0 + j, x = x0 + lane;
        re[j] = (y < H && x < W) ? a.r_ema[plane + (int64_t)y * W + x] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < SROWS; ++u) {
        const int r = wave + u * (SISR_BLOCK / 64);
        const int gy = at_mirror(y0 - P + r, H);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int c = lane + 64 * h;
            sv[u][h] = (r < SH && c < SC) ? rsr[(int64_t)gy * W + at_mirror(x0 - P + c, W)] : 0.f;
        }
    }
    // the patch weight: the sample's partials as shifted sums around the first one's mean, one term per thread (parts <= SISR_BLOCK),
    // added in a fixed order: every workgroup of a sample gets the same bits
    const double* st = a.stats + (int64_t)n * a.parts * 3;
    double s[3] = {0.0, 0.0, 0.0};
    if (tid < a.parts) {
        const double nb = st[3 * tid], dm = st[3 * tid + 1] - st[1];
        s[0] = nb;
        s[1] = nb * dm;
        s[2] = st[3 * tid + 2] + nb * dm * dm;
    }
#pragma unroll
    for (int u = 0; u < SROWS; ++u) {
        const int r = wave + u * (SISR_BLOCK / 64);
#pragma unroll
        for (int h = 0; h < 2; ++h)
            if (r < SH && lane + 64 * h < SC) tile[r * AT_SW + lane + 64 * h] = sv[u][h];
    }
    block_partial_sum<double, 3>(s);
    if (tid == 0) {
        const double m2 = s[2] - s[1] * s[1] / s[0];
        patch_weight = pow((m2 < 0.0 ? 0.0 : m2) / (s[0] - 1.0), 0.2);      // (a NaN stays a NaN)
    }
    __syncthreads();                                                          // the tile and the patch weight are visible

    // ---- window variance of the thread's AT_PX pixels in two passes: the mean (its error enters squared), then the squared deviations
    const float* src0 = tile + r0 * AT_SW + lane;
    float mean[AT_PX];
    double tot[AT_PX], dev[AT_PX];
    at_window<K, false>(src0, mean, tot);
#pragma unroll
    for (int j = 0; j < AT_PX; ++j) mean[j] = (float)tot[j] * (1.f / (float)(K * K));
    at_window<K, true>(src0, mean, dev);

    // ---- mask, map, the tile's sum
    const double pk = patch_weight / (double)(K * K - 1);
    double sum[1] = {0.0};
#pragma unroll
    for (int j = 0; j < AT_PX; ++j) {
        const int y = y0 + r0 + j, x = x0 + lane;
        if (y < H && x < W) {
            const float rs = tile[(r0 + j + P) * AT_SW + lane + P];
            const float m = rs < re[j] ? 0.f : (float)(pk * dev[j]);
            map[plane + (int64_t)y * W + x] = m;
            sum[0] = fma((double)m, (double)rs, sum[0]);
        }
    }
    if (with_loss) {
        block_partial_sum<double, 1>(sum);
        if (tid == 0) a.tile_sum[(int64_t)n * tiles + t] = sum[0];
    }
}

// ---- launch 3: one workgroup per sample ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SISR_BLOCK) artifact_finish_kernel(const double* __restrict__ tile_sum, int tiles, double scale,
                                                                     float* __restrict__ loss) {
    const double* ts = tile_sum + (int64_t)blockIdx.x * tiles;
    double s[1];
    fold_partials_double<1>(tiles, s, [&](int64_t i, double (&acc)[1]) { acc[0] += ts[i]; });
    if (threadIdx.x == 0) loss[blockIdx.x] = (float)(s[0] * scale);
}

// ---- backward: blockIdx.x = (n * C + c) * blocks_per_plane + block; kf = weight / (C H W) ------------------------------------------
template <bool VEC>
__global__ void __launch_bounds__(SISR_BLOCK) artifact_bwd_kernel(const float* __restrict__ sr, const float* __restrict__ gt,
                                                                  const float* __restrict__ map, const float* __restrict__ g, int C,
                                                                  int hw, int bpp, float kf, float* __restrict__ dsr,
                                                                  float* __restrict__ dgt) {
    const int pl = blockIdx.x / bpp, blk = blockIdx.x - pl * bpp;
    const int n = pl / C;
    const int q = blk * SISR_BLOCK + (int)threadIdx.x;
    if (4 * (int64_t)q >= hw) return;
    const int valid = min(4, hw - 4 * q);
    const float sc = g[n] * kf;
    const int64_t off = (int64_t)pl * hw + 4 * q;
    const f32x4 x = at_load4<VEC>(sr, off, valid), y = at_load4<VEC>(gt, off, valid);
    const f32x4 m = at_load4<VEC>(map, (int64_t)n * hw + 4 * q, valid);
    f32x4 d, e;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float diff = x[j] - y[j], tm = sc * m[j];
        d[j] = diff > 0.f ? tm : (diff < 0.f ? -tm : 0.f);
        e[j] = -d[j];
    }
    if (dsr) at_store4<VEC>(dsr, off, valid, d);
    if (dgt) at_store4<VEC>(dgt, off, valid, e);
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
static bool at_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// the shape checks every entry point shares
static int artifact_check_shape(int32_t N, int32_t C, int32_t H, int32_t W) {
    if (N < 1 || H < 1 || W < 1) return SISR_E_BADARG;
    if (C != 1 && C != 3) return SISR_E_UNSUPPORTED;
    if ((int64_t)H * W > INT32_MAX / C || N > INT32_MAX / ((int64_t)C * H * W)) return SISR_E_TOOBIG;
    return 0;
}

extern "C" int sisr_artifact_ws_floats(int32_t N, int32_t H, int32_t W) {
    ArtifactWs a;
    if (int e = artifact_ws(N, H, W, nullptr, a)) return e;
    return (int)a.floats;
}

extern "C" int sisr_artifact_fwd(const float* sr, const float* gt, const float* ema, int32_t N, int32_t C, int32_t H, int32_t W,
                                 int32_t ksize, float weight, void* ws, float* map, float* loss, void* stream) {
    if (!sr || !gt || !ema || !ws || !map || ((uintptr_t)ws & 7) || !std::isfinite(weight)) return SISR_E_BADARG;
    if (ksize < 3 || ksize > SISR_ARTIFACT_MAX_K || ksize % 2 == 0) return SISR_E_BADARG;
    if (int e = artifact_check_shape(N, C, H, W)) return e;
    if (H <= ksize / 2 || W <= ksize / 2) return SISR_E_UNSUPPORTED;
    ArtifactWs a;
    if (int e = artifact_ws(N, H, W, ws, a)) return e;
    const int hw = H * W, tiles = a.tiles_x * a.tiles_y;
    const bool vec = hw % 4 == 0 && at_aligned16(sr) && at_aligned16(gt) && at_aligned16(ema) && at_aligned16(a.r_sr);
    hipStream_t st = sisr_stream(stream);
    const dim3 grid1((unsigned)(N * a.parts)), block(SISR_BLOCK);
#define AT_RESIDUAL(CC, VV) hipLaunchKernelGGL((artifact_residual_kernel<CC, VV>), grid1, block, 0, st, sr, gt, ema, hw, a)
    if (C == 1) {
        if (vec) AT_RESIDUAL(1, true);
        else AT_RESIDUAL(1, false);
    } else {
        if (vec) AT_RESIDUAL(3, true);
        else AT_RESIDUAL(3, false);
    }
#undef AT_RESIDUAL
    SISR_CHECK_LAUNCH();
    const dim3 grid2((unsigned)(N * tiles));
    const int with_loss = loss ? 1 : 0;
#define AT_TILE(KK) hipLaunchKernelGGL(artifact_tile_kernel<KK>, grid2, block, 0, st, a, (int)H, (int)W, map, with_loss)
    switch (ksize) {
        case 3: AT_TILE(3); break;
        case 5: AT_TILE(5); break;
        case 7: AT_TILE(7); break;
        case 9: AT_TILE(9); break;
        default: AT_TILE(11); break;
    }
#undef AT_TILE
    SISR_CHECK_LAUNCH();
    if (loss) {
        hipLaunchKernelGGL(artifact_finish_kernel, dim3((unsigned)N), block, 0, st, (const double*)a.tile_sum, tiles,
                           (double)weight / ((double)C * H * W), loss);
        SISR_CHECK_LAUNCH();
    }
    return 0;
}

extern "C" int sisr_artifact_bwd(const float* sr, const float* gt, const float* map, const float* g, int32_t N, int32_t C, int32_t H,
                                 int32_t W, float weight, float* dsr, float* dgt, void* stream) {
    if (!sr || !gt || !map || !g || (!dsr && !dgt) || !std::isfinite(weight)) return SISR_E_BADARG;
    if (int e = artifact_check_shape(N, C, H, W)) return e;
    const int hw = H * W;
    const int bpp = ((hw + 3) / 4 + SISR_BLOCK - 1) / SISR_BLOCK;
    const int64_t wgs = (int64_t)N * C * bpp;              // at most N C H W / 4 + N C: below INT32_MAX
    if (wgs > INT32_MAX) return SISR_E_TOOBIG;
    const bool vec = hw % 4 == 0 && at_aligned16(sr) && at_aligned16(gt) && at_aligned16(map) && at_aligned16(dsr) && at_aligned16(dgt);
    const float kf = (float)((double)weight / ((double)C * H * W));
    hipStream_t st = sisr_stream(stream);
    if (vec)
        hipLaunchKernelGGL(artifact_bwd_kernel<true>, dim3((unsigned)wgs), dim3(SISR_BLOCK), 0, st, sr, gt, map, g, (int)C, hw, bpp, kf,
                           dsr, dgt);
    else
        hipLaunchKernelGGL(artifact_bwd_kernel<false>, dim3((unsigned)wgs), dim3(SISR_BLOCK), 0, st, sr, gt, map, g, (int)C, hw, bpp, kf,
                           dsr, dgt);
    SISR_CHECK_LAUNCH();
    return 0;
}
