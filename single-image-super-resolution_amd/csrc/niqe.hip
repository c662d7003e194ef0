// niqe.hip -- the no-reference image quality score NIQE (Mittal, Soundararajan, Bovik, IEEE SPL 2013) in the form of BasicSR's
// calculate_niqe: the 36 features of every block of an image and the score against a pristine model (the
// definition is stated once in sisr_hip.h).  Everything after the image is read is double.
// Features, four launches whatever N and the number of blocks are:
//   niqe_plane_kernel   the view (crop, range), the BT.601 studio-range luma, rint, cut to whole blocks -> plane 1 [N][h1][w1]
//   niqe_half_kernel    MATLAB's antialiased bicubic at exactly 1/2: 8 x 8 dyadic taps, the border mirrored with the edge pixel
//                       repeated -> plane 2 [N][h1 / 2][w1 / 2] (exact in double: integers times multiples of 2^-16)
//   niqe_block_kernel   once per scale, a workgroup of 1024 threads per block and sample: the block with a halo of 3 (clamped at the
//                       plane's border) in LDS; the window moments of every pixel ABOUT THAT PIXEL (the differences are exact, nothing cancels, and a
//                       constant neighbourhood gives an MSCN of exactly 0); the block's MSCN in LDS; then per field (the MSCN, its
//                       four circularly rolled products) five sums -- a thread adds its pixels in index order, the lanes of a wave by
//                       butterfly, the waves in index order -- and five threads fit the asymmetric generalised Gaussians side by side:
//                       a binary search of the rho table plus a neighbour comparison, the argmin of the definition
// Score, one launch: a workgroup per sample; which rows are free of NaNs (into the workspace), the column means with and without the
// incomplete rows (252 threads = 36 columns x 7 row splits, combined in split order), the covariance about the mean (32 rows at a time
// through LDS; every thread owns entries of the matrix and walks the rows in order), the factorisation S = L D L^T (Cholesky without
// its square roots) in LDS with d as one more row, so that the forward substitution rides on the updates.
// No atomics, plain vector stores, nothing read back by the host: the same bits on every call.
#include "sisr_dev.h"

#include <cmath>

#define NQ_F SISR_NIQE_FEATURES                      // 36
#define NQ_HALO 3
#define NQ_TABLE SISR_NIQE_TABLE                     // 9801
#define NQ_BT 1024                                   // threads of a block workgroup: four waves per SIMD over the one block a CU holds
#define NQ_BWAVES (NQ_BT / 64)
#define NQ_STAGE 8                                   // global loads of a thread in flight while a block is staged
#define NQ_CHUNK 32                                  // rows of the covariance staged at a time
#define NQ_ENTRIES ((NQ_F * NQ_F + SISR_BLOCK - 1) / SISR_BLOCK)      // matrix entries a thread may own
#define NQ_SPLITS 7                                  // row splits of the column means: 36 x 7 = 252 threads
static_assert(NQ_F * NQ_SPLITS <= SISR_BLOCK && NQ_F == 36, "one thread per (column, row split)");
static_assert(((SISR_NIQE_MAX_BLOCK + 2 * NQ_HALO) * (SISR_NIQE_MAX_BLOCK + 2 * NQ_HALO) + SISR_NIQE_MAX_BLOCK * SISR_NIQE_MAX_BLOCK + 8 * NQ_BWAVES + 32) * 8 <= 160 * 1024,
              "the staged block, its MSCN and the reduction slots fit the LDS of one workgroup");

struct NiqeGeom {
    int N, C, H, W, crop, block;
    int h1, w1, nby, nbx;                            // plane 1 and its blocks; plane 2 is h1 / 2 x w1 / 2 with blocks of block / 2
    double lo, k;                                    // v = (x - lo) k, k = 255 / (hi - lo)
    double g[7];                                     // the 1-D window
    double* plane1;
    double* plane2;
    int64_t bytes;
};

// -> 0 or a status code.  ws may be NULL (the size query)
static int niqe_geom(int64_t N, int64_t C, int64_t H, int64_t W, int64_t crop, int64_t block, void* ws, NiqeGeom& q) {
    if (N < 1 || H < 1 || W < 1 || crop < 0) return SISR_E_BADARG;
    if (block < 16 || block > SISR_NIQE_MAX_BLOCK || block % 2) return SISR_E_BADARG;
    if (H * W > INT32_MAX || N * C > INT32_MAX / (H * W)) return SISR_E_TOOBIG;
    const int64_t h = H - 2 * crop, w = W - 2 * crop;
    if (h < block || w < block) return SISR_E_UNSUPPORTED;
    q.N = (int)N; q.C = (int)C; q.H = (int)H; q.W = (int)W; q.crop = (int)crop; q.block = (int)block;
    q.nby = (int)(h / block); q.nbx = (int)(w / block);
    q.h1 = q.nby * q.block; q.w1 = q.nbx * q.block;
    const int64_t p1 = N * q.h1 * q.w1, p2 = p1 / 4, nb = (int64_t)q.nby * q.nbx;
    q.bytes = 8 * (p1 + p2) + ((4 * N * nb + 7) & ~(int64_t)7);          // the two planes, then the score's row flags
    q.plane1 = (double*)ws;
    q.plane2 = q.plane1 + p1;
    return 0;
}

// ---- launch 1: one thread per pixel of plane 1 ---------------------------------------------------------------------------------------
template <int C>
__global__ void __launch_bounds__(SISR_BLOCK) niqe_plane_kernel(const float* __restrict__ img, NiqeGeom q) {
#pragma clang fp contract(off)                       // the products and sums as written: rint sees the value the definition states
    const int64_t i = (int64_t)blockIdx.x * SISR_BLOCK + threadIdx.x;
    const int hw1 = q.h1 * q.w1;
    if (i >= (int64_t)q.N * hw1) return;
    const int n = (int)(i / hw1), r = (int)(i - (int64_t)n * hw1);
    const int y = r / q.w1, x = r - y * q.w1;
    const int64_t hw = (int64_t)q.H * q.W;
    const float* p = img + (int64_t)n * C * hw + (int64_t)(y + q.crop) * q.W + (x + q.crop);
    double v;
    if (C == 3) {
        const double R = ((double)p[0] - q.lo) * q.k, G = ((double)p[hw] - q.lo) * q.k, B = ((double)p[2 * hw] - q.lo) * q.k;
        v = 16.0 + ((65.481 * R + 128.553 * G) + 24.966 * B) / 255.0;
    } else {
        v = ((double)p[0] - q.lo) * q.k;
    }
    q.plane1[i] = rint(v);
}

// index of an 8-tap window past the axis: mirrored with the edge pixel repeated (-1 -> 0, L -> L - 1); the clamp serves no stored pixel
__device__ __forceinline__ int nq_mirror(int i, int L) {
    i = i < 0 ? -i - 1 : (i >= L ? 2 * L - 1 - i : i);
    return min(max(i, 0), L - 1);
}

// ---- launch 2: one thread per pixel of plane 2 ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SISR_BLOCK) niqe_half_kernel(NiqeGeom q) {
    const int h2 = q.h1 >> 1, w2 = q.w1 >> 1;
    const int64_t i = (int64_t)blockIdx.x * SISR_BLOCK + threadIdx.x;
    if (i >= (int64_t)q.N * h2 * w2) return;
    const int n = (int)(i / (h2 * w2)), r = (int)(i - (int64_t)n * h2 * w2);
    const int y = r / w2, x = r - y * w2;
    const double* __restrict__ src = q.plane1 + (int64_t)n * q.h1 * q.w1;
    const double wt[8] = {-3.0 / 256, -9.0 / 256, 29.0 / 256, 111.0 / 256, 111.0 / 256, 29.0 / 256, -9.0 / 256, -3.0 / 256};
    int xs[8];
#pragma unroll
    for (int b = 0; b < 8; ++b) xs[b] = nq_mirror(2 * x - 3 + b, q.w1);
    double acc = 0.0;
#pragma unroll
    for (int a = 0; a < 8; ++a) {
        const double* row = src + (int64_t)nq_mirror(2 * y - 3 + a, q.h1) * q.w1;
        double s = 0.0;
#pragma unroll
        for (int b = 0; b < 8; ++b) s += wt[b] * row[xs[b]];
        acc += wt[a] * s;
    }
    q.plane2[i] = acc;
}

// K sums of the workgroup, result in thread 0: the lanes by butterfly, the waves in index order through red [K][NQ_BWAVES]
template <int K>
__device__ __forceinline__ void nq_reduce(double (&v)[K], double* red) {
#pragma unroll
    for (int j = 0; j < K; ++j) v[j] = wave_sum(v[j]);
    __syncthreads();                                 // the slots' last readers are done
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int j = 0; j < K; ++j) red[j * NQ_BWAVES + (threadIdx.x >> 6)] = v[j];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < K; ++j) {
            v[j] = red[j * NQ_BWAVES];
#pragma unroll
            for (int w = 1; w < NQ_BWAVES; ++w) v[j] += red[j * NQ_BWAVES + w];
        }
    }
}

// The fit of one field from its five sums over cnt values: s[0], s[1] = sum of f^2 and count over f < 0; s[2], s[3] over f > 0;
// s[4] = sum |f|.  tables: [4][NQ_TABLE] = Gamma(1 / a), Gamma(2 / a), Gamma(3 / a), rho.  -> (alpha, m, beta_l, beta_r)
__device__ __forceinline__ void nq_fit(const double (&s)[5], double cnt, const double* __restrict__ tables, double (&out)[4]) {
    const double* __restrict__ rho = tables + 3 * NQ_TABLE;
    const double L = sqrt(s[0] / s[1]), R = sqrt(s[2] / s[3]);           // an empty side: 0 / 0, a NaN
    const double gam = L / R;
    const double ma = s[4] / cnt, r = ma * ma / ((s[0] + s[2]) / cnt);
    const double g2 = gam * gam + 1.0;
    const double rhat = r * (gam * gam * gam + 1.0) * (gam + 1.0) / (g2 * g2);
    int j = 0;
    if (fabs(rhat) < INFINITY) {                                         // a NaN or an infinity: every squared distance ties, the first wins
        int lo = 0, hi = NQ_TABLE;                                       // the first j with rho[j] >= rhat
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (rho[mid] < rhat) lo = mid + 1;
            else hi = mid;
        }
        j = lo < NQ_TABLE ? lo : NQ_TABLE - 1;
        if (lo > 0 && lo < NQ_TABLE) {
            const double da = rho[lo - 1] - rhat, db = rho[lo] - rhat;
            if (da * da <= db * db) j = lo - 1;                          // the first minimum
        }
    }
    const double alpha = __dadd_rn(0.2, __dmul_rn(0.001, (double)j));
    const double ga = tables[j], gb = tables[NQ_TABLE + j], gc = tables[2 * NQ_TABLE + j];
    const double t = sqrt(ga / gc);
    const double bl = L * t, br = R * t;
    out[0] = alpha;
    out[1] = (br - bl) * (gb / ga);
    out[2] = bl;
    out[3] = br;
}

// ---- launches 3 and 4: blockIdx.x = block of the sample, blockIdx.y = n; B = the block side at this scale -----------------------------
__global__ void __launch_bounds__(NQ_BT) niqe_block_kernel(const double* __restrict__ plane, int ph, int pw, int B, int nbx, NiqeGeom q,
                                                                const double* __restrict__ tables, double* __restrict__ feat,
                                                                float* __restrict__ sharp, int scale, uint32_t mT, uint32_t mB) {
    extern __shared__ double nq_lds[];      // mT, mB: fdiv_magic of T and B (i / T and i / B for i < 2^16 by one multiply-high)
    const int T = B + 2 * NQ_HALO, BB = B * B;
    double* tile = nq_lds;                           // [T][T]
    double* ms = tile + T * T;                       // [B][B]
    double* red = ms + BB;                           // [8][NQ_BWAVES]
    double* sums = red + 8 * NQ_BWAVES;               // [5 fields][5 sums]
    const int tid = threadIdx.x, n = blockIdx.y, b = blockIdx.x;
    const int by = b / nbx, bx = b - by * nbx;
    const double* __restrict__ src = plane + (int64_t)n * ph * pw;
    // staging: NQ_STAGE loads of a thread in flight before the first is waited for
    for (int i0 = tid; i0 < T * T; i0 += NQ_STAGE * NQ_BT) {
        double v[NQ_STAGE];
#pragma unroll
        for (int u = 0; u < NQ_STAGE; ++u) {
            const int i = min(i0 + u * NQ_BT, T * T - 1);       // (a slot past the tile re-reads its last element and is not stored)
            const int ty = fdiv(i, mT), tx = i - ty * T;
            const int gy = min(max(by * B + ty - NQ_HALO, 0), ph - 1), gx = min(max(bx * B + tx - NQ_HALO, 0), pw - 1);
            v[u] = src[(int64_t)gy * pw + gx];
        }
#pragma unroll
        for (int u = 0; u < NQ_STAGE; ++u)
            if (i0 + u * NQ_BT < T * T) tile[i0 + u * NQ_BT] = v[u];
    }
    __syncthreads();
    double first[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};                    // the MSCN field's five sums and the sum of sigma
    for (int i = tid; i < BB; i += NQ_BT) {
        const int y = fdiv(i, mB), x = i - y * B;
        const double* t0 = tile + y * T + x;
        const double c = t0[NQ_HALO * T + NQ_HALO];
        double m1 = 0.0, m2 = 0.0;
#pragma unroll
        for (int dy = 0; dy < 7; ++dy) {
#pragma unroll
            for (int dx = 0; dx < 7; ++dx) {
                const double d = t0[dy * T + dx] - c, w = q.g[dy] * q.g[dx];
                m1 = fma(w, d, m1);
                m2 = fma(w * d, d, m2);
            }
        }
        const double sigma = sqrt(fabs(m2 - m1 * m1));
        const double f = -m1 / (sigma + 1.0);
        ms[i] = f;
        const double f2 = f * f;
        if (f < 0.0) { first[0] += f2; first[1] += 1.0; }
        if (f > 0.0) { first[2] += f2; first[3] += 1.0; }
        first[4] += fabs(f);
        first[5] += sigma;
    }
    nq_reduce<6>(first, red);                        // (its barriers also publish the MSCN block)
    if (tid == 0) {
#pragma unroll
        for (int j = 0; j < 5; ++j) sums[j] = first[j];
        if (sharp && scale == 0) sharp[(int64_t)n * gridDim.x + b] = (float)(first[5] / (double)BB);
    }
    for (int k = 0; k < 4; ++k) {
        const int sy = k == 0 ? 0 : 1, sx = k == 1 ? 0 : (k == 3 ? -1 : 1);
        double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        for (int i = tid; i < BB; i += NQ_BT) {
            const int y = fdiv(i, mB), x = i - y * B;
            int yy = y - sy, xx = x - sx;            // numpy's roll: out[y][x] = in[(y - sy) mod B][(x - sx) mod B]
            yy += yy < 0 ? B : 0;
            xx += xx < 0 ? B : (xx >= B ? -B : 0);
            const double f = ms[i] * ms[yy * B + xx], f2 = f * f;
            if (f < 0.0) { s[0] += f2; s[1] += 1.0; }
            if (f > 0.0) { s[2] += f2; s[3] += 1.0; }
            s[4] += fabs(f);
        }
        nq_reduce<5>(s, red);
        if (tid == 0) {
#pragma unroll
            for (int j = 0; j < 5; ++j) sums[5 * (1 + k) + j] = s[j];
        }
    }
    __syncthreads();
    // the five fits side by side, a thread each: one table search's chain of dependent loads instead of five
    if (tid < 5) {
        const double s[5] = {sums[5 * tid], sums[5 * tid + 1], sums[5 * tid + 2], sums[5 * tid + 3], sums[5 * tid + 4]};
        double fit[4];
        nq_fit(s, (double)BB, tables, fit);
        double* o = feat + ((int64_t)n * gridDim.x + b) * NQ_F + 18 * scale;
        if (tid == 0) {
            o[0] = fit[0];
            o[1] = (fit[2] + fit[3]) * 0.5;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) o[2 + 4 * (tid - 1) + j] = fit[j];
        }
    }
}

// ---- the score: one workgroup per sample -----------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SISR_BLOCK) niqe_score_kernel(const double* __restrict__ feat, int nb, const double* __restrict__ mu_p,
                                                                const double* __restrict__ cov_p, int* __restrict__ rowok,
                                                                float* __restrict__ score) {
    __shared__ double part[NQ_SPLITS][NQ_F][4];      // per row split: sum and count of the non-NaN entries, of the complete rows
    __shared__ double mean_ok[NQ_F];
    __shared__ double S[NQ_F + 1][NQ_F + 1];       // rows 0 .. 35: (cov_p + cov_d) / 2; row 36: d = mu_p - mu_d
    __shared__ double rows[NQ_CHUNK][NQ_F + 1];
    __shared__ int n_ok;
    const int tid = threadIdx.x, n = blockIdx.x;
    const double* __restrict__ ft = feat + (int64_t)n * nb * NQ_F;
    int* __restrict__ ok = rowok + (int64_t)n * nb;
    for (int r = tid; r < nb; r += SISR_BLOCK) {
        int good = 1;
        for (int f = 0; f < NQ_F; ++f) good &= ft[(int64_t)r * NQ_F + f] == ft[(int64_t)r * NQ_F + f];
        ok[r] = good;
    }
    __syncthreads();                                 // the flags are visible to the workgroup
    const int per = (nb + NQ_SPLITS - 1) / NQ_SPLITS;
    if (tid < NQ_F * NQ_SPLITS) {
        const int f = tid % NQ_F, sp = tid / NQ_F;
        double sa = 0.0, ca = 0.0, so = 0.0, co = 0.0;
        for (int r = sp * per; r < min((sp + 1) * per, nb); ++r) {
            const double v = ft[(int64_t)r * NQ_F + f];
            if (v == v) { sa += v; ca += 1.0; }
            if (ok[r]) { so += v; co += 1.0; }
        }
        part[sp][f][0] = sa; part[sp][f][1] = ca; part[sp][f][2] = so; part[sp][f][3] = co;
    }
    __syncthreads();
    if (tid < NQ_F) {
        double t[4] = {0.0, 0.0, 0.0, 0.0};
        for (int sp = 0; sp < NQ_SPLITS; ++sp)
            for (int j = 0; j < 4; ++j) t[j] += part[sp][tid][j];
        S[NQ_F][tid] = mu_p[tid] - t[0] / t[1];      // nanmean: a column of NaNs alone gives 0 / 0
        mean_ok[tid] = t[2] / t[3];
        if (tid == 0) n_ok = (int)t[3];
    }
    __syncthreads();
    const int rows_ok = n_ok;
    // the covariance about the complete rows' mean: NQ_CHUNK rows at a time through LDS (deviations; an incomplete row as zeros, which
    // leave every sum as it is), entry (i, j >= i) by one thread, the rows in index order; then S = (cov_p + cov_d) / 2
    double acc[NQ_ENTRIES];
#pragma unroll
    for (int k = 0; k < NQ_ENTRIES; ++k) acc[k] = 0.0;
    for (int c0 = 0; c0 < nb; c0 += NQ_CHUNK) {
        const int cnt = min(NQ_CHUNK, nb - c0);
        for (int idx = tid; idx < cnt * NQ_F; idx += SISR_BLOCK) {
            const int r = idx / NQ_F, f = idx - r * NQ_F;
            const double v = ft[(int64_t)c0 * NQ_F + idx];
            rows[r][f] = ok[c0 + r] ? v - mean_ok[f] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < NQ_ENTRIES; ++k) {
            const int e = tid + k * SISR_BLOCK, i = e / NQ_F, j = e - i * NQ_F;
            if (e < NQ_F * NQ_F && j >= i)
                for (int r = 0; r < cnt; ++r) acc[k] = fma(rows[r][i], rows[r][j], acc[k]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < NQ_ENTRIES; ++k) {
        const int e = tid + k * SISR_BLOCK, i = e / NQ_F, j = e - i * NQ_F;
        if (e < NQ_F * NQ_F && j >= i) {
            const double c = acc[k] / (double)(rows_ok - 1);
            S[i][j] = (cov_p[i * NQ_F + j] + c) * 0.5;
            S[j][i] = (cov_p[j * NQ_F + i] + c) * 0.5;
        }
    }
    __syncthreads();
    // The factorisation in its square-root-free form, S = L D L^T, right-looking, one barrier per column.  d rides along as row 36 of
    // the matrix, so the forward substitution happens inside the updates: at column k row 36 holds (L^-1 d)_k D_k, and
    // d^T S^-1 d = sum_k S[36][k]^2 / D_k.  Every thread reads the same pivot: the exit on a pivot that is not > 0 (a NaN included)
    // is uniform.  Column k is only read at step k (its entries are final), entries right of it are updated.
    double q2 = 0.0;
    bool bad = rows_ok < 2;
    for (int k = 0; k < NQ_F && !bad; ++k) {
        const double p = S[k][k];
        if (!(p > 0.0)) {
            bad = true;
            break;
        }
        const double inv = 1.0 / p, yk = S[NQ_F][k];
        q2 = fma(yk * inv, yk, q2);
        for (int e = tid; e < (NQ_F + 1) * NQ_F; e += SISR_BLOCK) {
            const int i = e / NQ_F, j = e - i * NQ_F;
            if (j > k && i >= j) S[i][j] -= S[i][k] * inv * S[j][k];
        }
        __syncthreads();
    }
    if (tid == 0) score[n] = (float)sqrt(bad ? (double)NAN : q2);
}

// ---- host -------------------------------------------------------------------------------------------------------------------------------
extern "C" int64_t sisr_niqe_ws_bytes(int32_t N, int32_t H, int32_t W, int32_t crop, int32_t block) {
    NiqeGeom q;
    if (int e = niqe_geom(N, 1, H, W, crop, block, nullptr, q)) return e;
    return q.bytes;
}

extern "C" int sisr_niqe_features(const float* img, int32_t N, int32_t C, int32_t H, int32_t W, int32_t crop, float lo, float hi,
                                  int32_t block, const double* tables, void* ws, double* feat, float* sharp, void* stream) {
    if (!img || !tables || !ws || !feat || ((uintptr_t)ws & 7) || ((uintptr_t)feat & 7) || ((uintptr_t)tables & 7)) return SISR_E_BADARG;
    if (!std::isfinite(lo) || !std::isfinite(hi) || !(hi > lo)) return SISR_E_BADARG;
    if (N < 1 || H < 1 || W < 1 || crop < 0 || block < 16 || block > SISR_NIQE_MAX_BLOCK || block % 2) return SISR_E_BADARG;
    if (C != 1 && C != 3) return SISR_E_UNSUPPORTED;
    NiqeGeom q;
    if (int e = niqe_geom(N, C, H, W, crop, block, ws, q)) return e;
    if (N > 65535) return SISR_E_TOOBIG;                                 // a sample per grid row of the block launches
    q.lo = (double)lo;
    q.k = 255.0 / ((double)hi - (double)lo);
    double sum = 0.0;
    for (int k = 0; k < 7; ++k) {
        const double dk = (double)(k - 3), sg = 7.0 / 6.0;
        q.g[k] = exp(-(dk * dk) / (2.0 * sg * sg));
        sum += q.g[k];
    }
    for (int k = 0; k < 7; ++k) q.g[k] /= sum;
    hipStream_t st = sisr_stream(stream);
    const dim3 blk(SISR_BLOCK);
    const int64_t p1 = (int64_t)N * q.h1 * q.w1;
    const dim3 grid1((unsigned)((p1 + SISR_BLOCK - 1) / SISR_BLOCK)), grid2((unsigned)((p1 / 4 + SISR_BLOCK - 1) / SISR_BLOCK));
    if (C == 3) hipLaunchKernelGGL(niqe_plane_kernel<3>, grid1, blk, 0, st, img, q);
    else hipLaunchKernelGGL(niqe_plane_kernel<1>, grid1, blk, 0, st, img, q);
    SISR_CHECK_LAUNCH();
    hipLaunchKernelGGL(niqe_half_kernel, grid2, blk, 0, st, q);
    SISR_CHECK_LAUNCH();
    const dim3 gridb((unsigned)(q.nby * q.nbx), (unsigned)N);
    for (int s = 0; s < 2; ++s) {
        const int B = q.block >> s, T = B + 2 * NQ_HALO;
        const int lds = (T * T + B * B + 8 * NQ_BWAVES + 32) * 8;
        if (int e = sisr_launch<niqe_block_kernel>(gridb, dim3(NQ_BT), lds, 0, st, (const double*)(s ? q.plane2 : q.plane1), q.h1 >> s, q.w1 >> s, B,
                                                   q.nbx, q, tables, feat, sharp, s, fdiv_magic(T), fdiv_magic(B)))
            return e;
    }
    return 0;
}

extern "C" int sisr_niqe_score(const double* feat, int32_t N, int32_t nb, const double* mu_p, const double* cov_p, void* ws, float* score,
                               void* stream) {
    if (!feat || !mu_p || !cov_p || !ws || !score || ((uintptr_t)ws & 7) || ((uintptr_t)feat & 7) || ((uintptr_t)mu_p & 7) ||
        ((uintptr_t)cov_p & 7))
        return SISR_E_BADARG;
    if (N < 1 || nb < 1) return SISR_E_BADARG;
    if ((int64_t)N * nb > INT32_MAX / NQ_F) return SISR_E_TOOBIG;
    hipLaunchKernelGGL(niqe_score_kernel, dim3((unsigned)N), dim3(SISR_BLOCK), 0, sisr_stream(stream), feat, (int)nb, mu_p, cov_p, (int*)ws,
                       score);
    SISR_CHECK_LAUNCH();
    return 0;
}
