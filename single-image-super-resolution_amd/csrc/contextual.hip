// contextual.hip -- the contextual loss of Mechrez, Talmi and Zelnik-Manor (ECCV 2018) in its cosine form over the taps of a MaskedVGG
// feature vector, forward and backward.  fa (the generator side), fb (the target, a constant of the loss): fp32
// [B][total], tap l is columns [off_l, off_l + C_l P_l) of every row in NCHW order, X[n] / Y[n] that slice of fa / fb as C_l x P_l, column
// i the feature point x_i.  Per tap:
//   mu = the channel-wise mean of Y over the batch and all points        x^_i = (x_i - mu) / max(|x_i - mu|, 1e-12),  y^_j likewise
//   S_ij = x^_i . y^_j     d_ij = 1 - S_ij     m_i = min_j d_ij     w_ij = exp((1 - d_ij / (m_i + 1e-5)) / h)     Z_i = sum_j w_ij
//   CX_ij = w_ij / Z_i     c_j = max_i CX_ij     CX[n] = (1 / P) sum_j c_j     T_l = (1 / B) sum_n -log(CX[n] + 1e-5)
//   loss = weight sum_l w_l T_l.       Ties of the min and of the max take the lowest index.
// Launches (none depends on B; every one walks all taps and samples from a table passed by value):
//   cx_mean_kernel     one workgroup per (tap, channel): the sum of Y's channel over batch and points in double in a fixed order -> mu
//   cx_norm_kernel     |x - mu| of every point of both inputs, the squares added over the channels in double: lanes along p, which is
//                      contiguous (the channels are P apart); the four waves of a workgroup take every fourth channel of 64 points and
//                      meet in LDS in wave order
//   cx_sim_kernel      S[n] = X^^T Y^ on v_mfma_f32_32x32x2_f32 with K = C: a workgroup owns 64 x 64 of S, a wave one 32 x 32 tile; chunks
//                      of CS_KC channels of both operands are centred (x - mu) on their way into LDS as [channel][point] -- both operands
//                      want lanes along the point, which is contiguous in memory -- ragged C and P are zeros in LDS; the two 1 / norm
//                      factors scale the tile in the epilogue, so neither x^ nor y^ exists in memory
//   cx_row_kernel      one workgroup per row i: the row of S in registers (P <= SISR_CX_MAX_POINTS = 9 x 256), m_i and j*(i), then Z_i
//                      in double in a fixed order
//   cx_col_kernel      one workgroup per (sample, 64 columns): c_j = max_i w_ij / Z_i and i*(j), w recomputed from S by the row pass's
//                      own function (the same bits), loads coalesced along j; one double partial of sum_j c_j per workgroup
//   cx_finish_kernel   one workgroup: CX[n], the per-tap terms, the scalar
//   backward: cx_sim_kernel again (nothing of size P^2 is kept between forward and backward), then
//   cx_bwd_row_kernel  one workgroup per row i: r_i in gather form (the row scans the i* table), q_i, and T_ij = -dloss / dd_ij times
//                      1 / |y_j - mu| over S in place
//   cx_bwd_mm_kernel   dloss / dx^ = Y^ T^T on the same instruction with K = P: both operands have K contiguous in memory, so they
//                      go through LDS as [row][k] with pitch 33 and are read with lanes along the row
//   cx_bwd_proj_kernel the normalisation's projection (v - x^ (x^ . v)) / |x - mu|, 0 under 1e-12, in the norm pass's thread layout
// No atomics, every sum in a fixed order, every output element stored once, the same bits on every call, nothing read back by the host.
#include "sisr_dev.h"

#include <algorithm>
#include <cmath>

#define CX_PER (SISR_CX_MAX_POINTS / SISR_BLOCK)      // elements of a row a thread of the row passes holds
#define CS_KC 32                                      // channels per staged chunk of the similarity kernel (2 x 8 KB of LDS)
#define CB_KC 32                                      // points per staged chunk of the backward product
#define CB_PITCH (CB_KC + 1)
#define CX_EPS 1e-5f
#define CX_TINY 1e-12f
static_assert(SISR_BLOCK == 256 && SISR_CX_MAX_POINTS % SISR_BLOCK == 0, "the row passes hold a row in 256 x CX_PER registers");

struct CxTap {
    int C, P;
    int nt;                           // tiles of 64 points
    int ntc;                          // tiles of 64 channels
    float w;
    int64_t off;                      // first column of the tap
    int64_t mu;                       // floats before the tap's mu in the tables
    int64_t pt;                       // elements before the tap's [B][P] block in every per-point table
    int64_t s;                        // floats before the tap's [B][P][P] block in S
};
struct CxTable {
    int n, B;
    int64_t total;
    int64_t n_mu, n_pt, n_s;          // sum_l C_l, B sum_l P_l, B sum_l P_l^2
    int blk_mean[SISR_PERCEP_MAX_TAPS + 1], blk_pt[SISR_PERCEP_MAX_TAPS + 1], blk_sim[SISR_PERCEP_MAX_TAPS + 1],
        blk_row[SISR_PERCEP_MAX_TAPS + 1], blk_col[SISR_PERCEP_MAX_TAPS + 1], blk_mm[SISR_PERCEP_MAX_TAPS + 1];
    CxTap t[SISR_PERCEP_MAX_TAPS];
};
// the tables: mu [n_mu], then seven per-point tables of n_pt elements each
struct CxTab {
    float *mu, *na, *nb, *m, *Z, *c;
    int *jstar, *istar;
};

__device__ __forceinline__ int cx_tap_of(const int* blk0, int n, int b) {
    int l = 0;
    while (l + 1 < n && b >= blk0[l + 1]) ++l;
    return l;
}

__host__ __device__ inline CxTab cx_tab(const CxTable& tb, void* tab) {
    CxTab q;
    float* f = (float*)tab;
    q.mu = f;
    q.na = f + tb.n_mu;
    q.nb = q.na + tb.n_pt;
    q.m = q.nb + tb.n_pt;
    q.Z = q.m + tb.n_pt;
    q.c = q.Z + tb.n_pt;
    q.jstar = (int*)(q.c + tb.n_pt);
    q.istar = q.jstar + tb.n_pt;
    return q;
}

// (value, index) pairs of an arg-min / arg-max: a NaN wins over every number, ties take the lowest index.  Commutative and associative,
// so the order of a reduction does not matter
template <bool MAX>
__device__ __forceinline__ bool cx_wins(float v1, int i1, float v2, int i2) {
    const bool n1 = v1 != v1, n2 = v2 != v2;
    if (n1 || n2) return n1 && (!n2 || i1 < i2);
    return (MAX ? v1 > v2 : v1 < v2) || (v1 == v2 && i1 < i2);
}
template <bool MAX>
__device__ __forceinline__ void cx_arg_block(float& v, int& i, float* sv, int* si) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float v2 = __shfl_xor(v, o);
        const int i2 = __shfl_xor(i, o);
        if (cx_wins<MAX>(v2, i2, v, i)) { v = v2; i = i2; }
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = v; si[threadIdx.x >> 6] = i; }
    __syncthreads();
    v = sv[0];
    i = si[0];
#pragma unroll
    for (int w = 1; w < SISR_BLOCK / 64; ++w)
        if (cx_wins<MAX>(sv[w], si[w], v, i)) { v = sv[w]; i = si[w]; }
}
// a workgroup's sum in double: the lanes of a wave by the butterfly, the waves in index order; valid in all threads
__device__ __forceinline__ double cx_sum_block(double v, double* sd) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sd[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = sd[0];
#pragma unroll
    for (int w = 1; w < SISR_BLOCK / 64; ++w) t += sd[w];
    return t;
}

// w_ij of the row pass, the column pass and the backward: one text, no contraction, so that the three form the same bits
__device__ __forceinline__ float cx_weight(float d, float den, float inv_h) {
#pragma clang fp contract(off)
    const float dt = d / den;
    const float a = (1.f - dt) * inv_h;
    return expf(a);
}

// ---- mu: blockIdx.x = blk_mean[l] + channel -------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SISR_BLOCK) cx_mean_kernel(const float* __restrict__ fb, CxTable tb, float* __restrict__ tab) {
    const int l = cx_tap_of(tb.blk_mean, tb.n, (int)blockIdx.x);
    const CxTap t = tb.t[l];
    const int c = (int)blockIdx.x - tb.blk_mean[l];
    const float* __restrict__ Y = fb + t.off + (int64_t)c * t.P;
    const int64_t count = (int64_t)tb.B * t.P;
    double s[1];
    fold_partials_double<1>(count, s, [&](int64_t i, double (&acc)[1]) {
        const int64_t n = i / t.P;
        acc[0] += (double)Y[n * tb.total + (i - n * t.P)];
    });
    if (threadIdx.x == 0) cx_tab(tb, tab).mu[t.mu + c] = (float)(s[0] / (double)count);
}

// ---- norms: blockIdx.x = blk_pt[l] + ((x * B + n) * nt + tile of 64 points); thread = (point tid & 63, channel group tid >> 6): the groups
// take every fourth channel each and meet in LDS in group order ----------------------------------------------------------------------------
__global__ void __launch_bounds__(SISR_BLOCK) cx_norm_kernel(const float* __restrict__ fa, const float* __restrict__ fb, CxTable tb,
                                                             float* __restrict__ tab) {
    __shared__ double part[SISR_BLOCK];
    const int l = cx_tap_of(tb.blk_pt, tb.n, (int)blockIdx.x);
    const CxTap t = tb.t[l];
    int r = (int)blockIdx.x - tb.blk_pt[l];
    const int pb = r % t.nt;
    r /= t.nt;
    const int n = r % tb.B, x = r / tb.B;
    const int p = pb * 64 + ((int)threadIdx.x & 63), grp = (int)threadIdx.x >> 6;
    const CxTab q = cx_tab(tb, tab);
    const float* __restrict__ mu = q.mu + t.mu;
    double s = 0.0;
    if (p < t.P) {
        const float* __restrict__ F = (x ? fb : fa) + (int64_t)n * tb.total + t.off + p;
#pragma unroll 4
        for (int c = grp; c < t.C; c += SISR_BLOCK / 64) {
            const float v = F[(int64_t)c * t.P] - mu[c];
            s += (double)v * (double)v;
        }
    }
    part[threadIdx.x] = s;
    __syncthreads();
    if (grp == 0 && p < t.P)
        (x ? q.nb : q.na)[t.pt + (int64_t)n * t.P + p] = (float)sqrt(((part[threadIdx.x] + part[threadIdx.x + 64]) + part[threadIdx.x + 128]) +
                                                                     part[threadIdx.x + 192]);
}

// ---- S: blockIdx.x = blk_sim[l] + ((n * nt + ti) * nt + tj); wave w owns rows 32 (w & 1) .., columns 32 (w >> 1) .. of the 64 x 64 -----------
__global__ void __launch_bounds__(SISR_BLOCK) cx_sim_kernel(const float* __restrict__ fa, const float* __restrict__ fb, CxTable tb,
                                                            const float* __restrict__ tab, float* __restrict__ S) {
    __shared__ float sa[CS_KC * 64], sb[CS_KC * 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, kk = lane >> 5;
    const int l = cx_tap_of(tb.blk_sim, tb.n, (int)blockIdx.x);
    const CxTap t = tb.t[l];
    int r = (int)blockIdx.x - tb.blk_sim[l];
    const int tj = r % t.nt;
    r /= t.nt;
    const int ti = r % t.nt, n = r / t.nt;
    const int i0 = ti * 64, j0 = tj * 64;
    const CxTab q = cx_tab(tb, const_cast<float*>(tab));
    const float* __restrict__ X = fa + (int64_t)n * tb.total + t.off;
    const float* __restrict__ Y = fb + (int64_t)n * tb.total + t.off;
    const float* __restrict__ mu = q.mu + t.mu;
    const int srow = tid >> 6, scol = tid & 63;
    const bool iok = i0 + scol < t.P, jok = j0 + scol < t.P;
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    for (int c0 = 0; c0 < t.C; c0 += CS_KC) {
        if (c0) __syncthreads();                                   // the previous chunk has been multiplied
        float va[CS_KC / 4], vb[CS_KC / 4];
#pragma unroll
        for (int u = 0; u < CS_KC / 4; ++u) {
            const int c = c0 + srow + 4 * u;
            va[u] = vb[u] = 0.f;
            if (c < t.C) {
                const float m = mu[c];
                if (iok) va[u] = X[(int64_t)c * t.P + i0 + scol] - m;
                if (jok) vb[u] = Y[(int64_t)c * t.P + j0 + scol] - m;
            }
        }
#pragma unroll
        for (int u = 0; u < CS_KC / 4; ++u) {
            sa[(srow + 4 * u) * 64 + scol] = va[u];
            sb[(srow + 4 * u) * 64 + scol] = vb[u];
        }
        __syncthreads();
        // steps of two channels in channel order; the row behind an odd tail is zeros
        const int steps = (min(CS_KC, t.C - c0) + 1) >> 1;
        const float* ap = sa + kk * 64 + (wave & 1) * 32 + l31;
        const float* bp = sb + kk * 64 + (wave >> 1) * 32 + l31;
        for (int st = 0; st < steps; ++st) acc = mfma32(ap[2 * st * 64], bp[2 * st * 64], acc);
    }
    // acc[reg]: row mfma_row(reg, lane), column l31
    const int j = j0 + (wave >> 1) * 32 + l31;
    if (j >= t.P) return;
    const float* __restrict__ na = q.na + t.pt + (int64_t)n * t.P;
    const float ib = 1.f / fmaxf(q.nb[t.pt + (int64_t)n * t.P + j], CX_TINY);
    float* __restrict__ out = S + t.s + (int64_t)n * t.P * t.P;
#pragma unroll
    for (int u = 0; u < 16; ++u) {
        const int i = i0 + (wave & 1) * 32 + mfma_row(u, lane);
        if (i < t.P) {
            const float ia = 1.f / fmaxf(na[i], CX_TINY);
            out[(int64_t)i * t.P + j] = (acc[u] * ia) * ib;
        }
    }
}

// ---- rows: blockIdx.x = blk_row[l] + n * P + i ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SISR_BLOCK) cx_row_kernel(const float* __restrict__ S, CxTable tb, float inv_h, float* __restrict__ tab) {
    __shared__ float sv[SISR_BLOCK / 64];
    __shared__ int si[SISR_BLOCK / 64];
    __shared__ double sd[SISR_BLOCK / 64];
    const int tid = threadIdx.x;
    const int l = cx_tap_of(tb.blk_row, tb.n, (int)blockIdx.x);
    const CxTap t = tb.t[l];
    const int64_t row = (int64_t)((int)blockIdx.x - tb.blk_row[l]);          // n * P + i
    const float* __restrict__ s = S + t.s + row * t.P;
    float d[CX_PER];
    float best = INFINITY;
    int arg = INT32_MAX;
#pragma unroll
    for (int k = 0; k < CX_PER; ++k) {
        const int j = tid + SISR_BLOCK * k;
        d[k] = 0.f;
        if (j < t.P) {
            d[k] = 1.f - s[j];
            if (cx_wins<false>(d[k], j, best, arg)) { best = d[k]; arg = j; }
        }
    }
    cx_arg_block<false>(best, arg, sv, si);
    const float den = best + CX_EPS;
    double z = 0.0;
#pragma unroll
    for (int k = 0; k < CX_PER; ++k)
        if (tid + SISR_BLOCK * k < t.P) z += (double)cx_weight(d[k], den, inv_h);
    z = cx_sum_block(z, sd);
    if (tid == 0) {
        const CxTab q = cx_tab(tb, tab);
        q.m[t.pt + row] = best;
        q.jstar[t.pt + row] = arg;
        q.Z[t.pt + row] = (float)z;
    }
}

// ---- columns: blockIdx.x = blk_col[l] + n * nt + tj; thread = (column tid & 63, row group tid >> 6) ----------------------------------------------
__global__ void __launch_bounds__(SISR_BLOCK) cx_col_kernel(const float* __restrict__ S, CxTable tb, float inv_h, float* __restrict__ tab,
                                                            double* __restrict__ part) {
    __shared__ float sv[SISR_BLOCK];
    __shared__ int si[SISR_BLOCK];
    const int tid = threadIdx.x, col = tid & 63, rg = tid >> 6;
    const int l = cx_tap_of(tb.blk_col, tb.n, (int)blockIdx.x);
    const CxTap t = tb.t[l];
    const int r = (int)blockIdx.x - tb.blk_col[l];
    const int tj = r % t.nt, n = r / t.nt;
    const int j = tj * 64 + col;
    const CxTab q = cx_tab(tb, tab);
    const float* __restrict__ s = S + t.s + (int64_t)n * t.P * t.P;
    const float* __restrict__ m = q.m + t.pt + (int64_t)n * t.P;
    const float* __restrict__ Z = q.Z + t.pt + (int64_t)n * t.P;
    float best = -INFINITY;
    int arg = INT32_MAX;
    if (j < t.P) {
        for (int i = rg; i < t.P; i += SISR_BLOCK / 64) {
            const float cx = cx_weight(1.f - s[(int64_t)i * t.P + j], m[i] + CX_EPS, inv_h) / Z[i];
            if (cx_wins<true>(cx, i, best, arg)) { best = cx; arg = i; }
        }
    }
    sv[tid] = best;
    si[tid] = arg;
    __syncthreads();
    if (tid < 64) {
#pragma unroll
        for (int g = 1; g < SISR_BLOCK / 64; ++g)
            if (cx_wins<true>(sv[tid + 64 * g], si[tid + 64 * g], best, arg)) { best = sv[tid + 64 * g]; arg = si[tid + 64 * g]; }
        if (j < t.P) {
            q.c[t.pt + (int64_t)n * t.P + j] = best;
            q.istar[t.pt + (int64_t)n * t.P + j] = arg;
        }
        const double sum = wave_sum(j < t.P ? (double)best : 0.0);
        if (tid == 0) part[blockIdx.x] = sum;
    }
}

// ---- CX[n], the terms and the scalar: one workgroup ----------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SISR_BLOCK) cx_finish_kernel(CxTable tb, const double* __restrict__ part, double weight,
                                                               float* __restrict__ cx, float* __restrict__ terms, float* __restrict__ loss) {
    double tot = 0.0;
    for (int l = 0; l < tb.n; ++l) {
        const CxTap t = tb.t[l];
        const double* p = part + tb.blk_col[l];
        double s[1];
        fold_partials_double<1>(tb.B, s, [&](int64_t n, double (&acc)[1]) {
            double c = p[n * t.nt];
            for (int k = 1; k < t.nt; ++k) c += p[n * t.nt + k];
            const float v = (float)(c / (double)t.P);
            cx[(int64_t)l * tb.B + n] = v;
            acc[0] += -log((double)v + 1e-5);
        });
        const double term = s[0] / (double)tb.B;
        if (threadIdx.x == 0 && terms) terms[l] = (float)term;
        tot += (double)t.w * term;
        __syncthreads();                                           // the fold's LDS is free again
    }
    if (threadIdx.x == 0) loss[0] = (float)(weight * tot);
}

// ---- backward rows: blockIdx.x = blk_row[l] + n * P + i; S -> T_ij / |y_j - mu| in place ----------------------------------------------------------
__global__ void __launch_bounds__(SISR_BLOCK) cx_bwd_row_kernel(float* __restrict__ S, CxTable tb, float inv_h, const float* __restrict__ tab,
                                                                const float* __restrict__ cx, const float* __restrict__ g, double weight) {
    __shared__ double sd[SISR_BLOCK / 64];
    const int tid = threadIdx.x;
    const int l = cx_tap_of(tb.blk_row, tb.n, (int)blockIdx.x);
    const CxTap t = tb.t[l];
    const int64_t row = (int64_t)((int)blockIdx.x - tb.blk_row[l]);
    const int n = (int)(row / t.P), i = (int)(row - (int64_t)n * t.P);
    const CxTab q = cx_tab(tb, const_cast<float*>(tab));
    float* __restrict__ s = S + t.s + row * t.P;
    const int64_t pn = t.pt + (int64_t)n * t.P;
    const float den = q.m[pn + i] + CX_EPS, z = q.Z[pn + i];
    const int js = q.jstar[pn + i];
    // gamma_n / P
    const float gp = (float)(-(double)g[0] * weight * (double)t.w / ((double)tb.B * ((double)cx[(int64_t)l * tb.B + n] + 1e-5)) / (double)t.P);
    float d[CX_PER], c[CX_PER];
    bool top[CX_PER];
    double rs = 0.0;
#pragma unroll
    for (int k = 0; k < CX_PER; ++k) {
        const int j = tid + SISR_BLOCK * k;
        d[k] = c[k] = 0.f;
        top[k] = false;
        if (j < t.P) {
            d[k] = 1.f - s[j];
            c[k] = cx_weight(d[k], den, inv_h) / z;
            top[k] = q.istar[pn + j] == i;
            if (top[k]) rs += (double)c[k];
        }
    }
    const float r = gp * (float)cx_sum_block(rs, sd);               // r_i = sum_j G_ij CX_ij, G_ij = gamma / P where i = i*(j)
    double qs = 0.0;
#pragma unroll
    for (int k = 0; k < CX_PER; ++k) {
        c[k] = -c[k] * ((top[k] ? gp : 0.f) - r) * inv_h;           // E_ij
        qs += (double)c[k] * (double)d[k];
    }
    const float qi = (float)cx_sum_block(qs, sd);
    const float pick = qi / (den * den);
#pragma unroll
    for (int k = 0; k < CX_PER; ++k) {
        const int j = tid + SISR_BLOCK * k;
        if (j < t.P) {
            const float dd = c[k] / den - (j == js ? pick : 0.f);
            s[j] = -dd * (1.f / fmaxf(q.nb[pn + j], CX_TINY));
        }
    }
}

// ---- dloss / dx^ = Y^ T^T: blockIdx.x = blk_mm[l] + ((n * ntc + tc) * nt + ti); wave w owns channels 32 (w & 1) .., points 32 (w >> 1) .. ----------
__global__ void __launch_bounds__(SISR_BLOCK) cx_bwd_mm_kernel(const float* __restrict__ fb, const float* __restrict__ T, CxTable tb,
                                                               const float* __restrict__ tab, float* __restrict__ dxh) {
    __shared__ float sy[64 * CB_PITCH], st[64 * CB_PITCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, kk = lane >> 5;
    const int l = cx_tap_of(tb.blk_mm, tb.n, (int)blockIdx.x);
    const CxTap t = tb.t[l];
    int r = (int)blockIdx.x - tb.blk_mm[l];
    const int ti = r % t.nt;
    r /= t.nt;
    const int tc = r % t.ntc, n = r / t.ntc;
    const int c0 = tc * 64, i0 = ti * 64;
    const float* __restrict__ Y = fb + (int64_t)n * tb.total + t.off;
    const float* __restrict__ Tn = T + t.s + (int64_t)n * t.P * t.P;
    const float* __restrict__ mu = cx_tab(tb, const_cast<float*>(tab)).mu + t.mu;
    const int srow = tid >> 5, sk = tid & 31;
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    for (int j0 = 0; j0 < t.P; j0 += CB_KC) {
        if (j0) __syncthreads();
        float vy[8], vt[8];
        const int j = j0 + sk;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int rr = srow + 8 * u;
            vy[u] = vt[u] = 0.f;
            if (j < t.P) {
                if (c0 + rr < t.C) vy[u] = Y[(int64_t)(c0 + rr) * t.P + j] - mu[c0 + rr];
                if (i0 + rr < t.P) vt[u] = Tn[(int64_t)(i0 + rr) * t.P + j];
            }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            sy[(srow + 8 * u) * CB_PITCH + sk] = vy[u];
            st[(srow + 8 * u) * CB_PITCH + sk] = vt[u];
        }
        __syncthreads();
        const int steps = (min(CB_KC, t.P - j0) + 1) >> 1;
        const float* ap = sy + ((wave & 1) * 32 + l31) * CB_PITCH + kk;
        const float* bp = st + ((wave >> 1) * 32 + l31) * CB_PITCH + kk;
        for (int s = 0; s < steps; ++s) acc = mfma32(ap[2 * s], bp[2 * s], acc);
    }
    const int i = i0 + (wave >> 1) * 32 + l31;
    if (i >= t.P) return;
    float* __restrict__ out = dxh + (int64_t)n * tb.total + t.off;
#pragma unroll
    for (int u = 0; u < 16; ++u) {
        const int c = c0 + (wave & 1) * 32 + mfma_row(u, lane);
        if (c < t.C) out[(int64_t)c * t.P + i] = acc[u];
    }
}

// ---- the projection: blockIdx.x = blk_pt[l] + (n * nt + tile of 64 points), the first B * nt workgroups of every tap's walk; thread =
// (point tid & 63, channel group tid >> 6) as in the norm pass ----------------------------------------------------------------------------------
__global__ void __launch_bounds__(SISR_BLOCK) cx_bwd_proj_kernel(const float* __restrict__ fa, const float* __restrict__ dxh, CxTable tb,
                                                                 const float* __restrict__ tab, float* __restrict__ dfa) {
    __shared__ double part[SISR_BLOCK];
    const int l = cx_tap_of(tb.blk_pt, tb.n, (int)blockIdx.x);
    const CxTap t = tb.t[l];
    const int r = (int)blockIdx.x - tb.blk_pt[l];
    const int pb = r % t.nt, n = r / t.nt;
    if (n >= tb.B) return;                                         // the walk has a second half for fb in the norm pass (whole workgroups)
    const int p = pb * 64 + ((int)threadIdx.x & 63), grp = (int)threadIdx.x >> 6;
    const bool live = p < t.P;
    const CxTab q = cx_tab(tb, const_cast<float*>(tab));
    const int64_t base = (int64_t)n * tb.total + t.off + (live ? p : 0);
    const float* __restrict__ X = fa + base;
    const float* __restrict__ V = dxh + base;
    float* __restrict__ O = dfa + base;
    const float* __restrict__ mu = q.mu + t.mu;
    const float na = live ? q.na[t.pt + (int64_t)n * t.P + p] : 1.f;
    const bool zero = na < CX_TINY;
    const float inv = 1.f / (zero ? 1.f : na);
    double dot = 0.0;
    if (live && !zero) {
#pragma unroll 4
        for (int c = grp; c < t.C; c += SISR_BLOCK / 64) dot += (double)((X[(int64_t)c * t.P] - mu[c]) * inv) * (double)V[(int64_t)c * t.P];
    }
    part[threadIdx.x] = dot;
    __syncthreads();
    if (!live) return;
    const int pl = (int)threadIdx.x & 63;
    const float dt = (float)(((part[pl] + part[pl + 64]) + part[pl + 128]) + part[pl + 192]);
#pragma unroll 4
    for (int c = grp; c < t.C; c += SISR_BLOCK / 64) {
        const float xh = (X[(int64_t)c * t.P] - mu[c]) * inv;
        O[(int64_t)c * t.P] = zero ? 0.f : (V[(int64_t)c * t.P] - xh * dt) * inv;
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------------------------
// the table of a call -> 0 or a status code.  `total`: < 0 skips the sum check (the size query)
static int cx_table(int32_t B, int64_t total, int32_t n_taps, const int32_t* shapes, const float* layer_w, CxTable& tb) {
    if (!shapes || B < 1 || n_taps < 1 || n_taps > SISR_PERCEP_MAX_TAPS) return SISR_E_BADARG;
    tb.n = n_taps;
    tb.B = B;
    tb.total = total;
    int64_t off = 0, mu = 0, pt = 0, s = 0, bm = 0, bp = 0, bs = 0, br = 0, bc = 0, bmm = 0;
    for (int l = 0; l < n_taps; ++l) {
        const int64_t C = shapes[3 * l], H = shapes[3 * l + 1], W = shapes[3 * l + 2];
        if (C < 1 || H < 1 || W < 1) return SISR_E_BADARG;
        if (H * W > SISR_CX_MAX_POINTS || C > (1 << 20)) return SISR_E_TOOBIG;
        CxTap& t = tb.t[l];
        t.C = (int)C;
        t.P = (int)(H * W);
        t.nt = (t.P + 63) / 64;
        t.ntc = (t.C + 63) / 64;
        t.w = layer_w ? layer_w[l] : 1.f;
        t.off = off;
        t.mu = mu;
        t.pt = pt;
        t.s = s;
        tb.blk_mean[l] = (int)bm;
        tb.blk_pt[l] = (int)bp;
        tb.blk_sim[l] = (int)bs;
        tb.blk_row[l] = (int)br;
        tb.blk_col[l] = (int)bc;
        tb.blk_mm[l] = (int)bmm;
        off += C * t.P;
        mu += C;
        pt += (int64_t)B * t.P;
        s += (int64_t)B * t.P * t.P;
        bm += C;
        bp += 2 * (int64_t)B * t.nt;
        bs += (int64_t)B * t.nt * t.nt;
        br += (int64_t)B * t.P;
        bc += (int64_t)B * t.nt;
        bmm += (int64_t)B * t.ntc * t.nt;
        if (off > ((int64_t)1 << 40) || s > ((int64_t)1 << 40) || std::max(std::max(std::max(bm, bp), std::max(bs, br)), bmm) > INT32_MAX / 2)
            return SISR_E_TOOBIG;
    }
    if (total >= 0 && off != total) return SISR_E_BADARG;
    tb.n_mu = mu;
    tb.n_pt = pt;
    tb.n_s = s;
    tb.blk_mean[n_taps] = (int)bm;
    tb.blk_pt[n_taps] = (int)bp;
    tb.blk_sim[n_taps] = (int)bs;
    tb.blk_row[n_taps] = (int)br;
    tb.blk_col[n_taps] = (int)bc;
    tb.blk_mm[n_taps] = (int)bmm;
    return 0;
}

static int64_t cx_part_bytes(const CxTable& tb) { return 8 * (((int64_t)tb.blk_col[tb.n] + 1) & ~(int64_t)1); }

extern "C" int64_t sisr_cx_ws_bytes(int32_t B, int32_t n_taps, const int32_t* shapes, int32_t which) {
    CxTable tb;
    if (int e = cx_table(B, -1, n_taps, shapes, nullptr, tb)) return e;
    const CxTap& last = tb.t[n_taps - 1];
    const int64_t total = last.off + (int64_t)last.C * last.P;
    switch (which) {
        case SISR_CX_WS_TABLES: return 4 * (tb.n_mu + 7 * tb.n_pt);
        case SISR_CX_WS_SIM: return 4 * tb.n_s;
        case SISR_CX_WS_FWD: return cx_part_bytes(tb) + 4 * tb.n_s;
        case SISR_CX_WS_BWD: return 4 * (tb.n_s + (int64_t)B * total);
    }
    return SISR_E_BADARG;
}

// mu, the norms and S: three launches
static int cx_similarity(const float* fa, const float* fb, const CxTable& tb, float* tab, float* S, hipStream_t st) {
    const dim3 block(SISR_BLOCK);
    hipLaunchKernelGGL(cx_mean_kernel, dim3((unsigned)tb.blk_mean[tb.n]), block, 0, st, fb, tb, tab);
    SISR_CHECK_LAUNCH();
    hipLaunchKernelGGL(cx_norm_kernel, dim3((unsigned)tb.blk_pt[tb.n]), block, 0, st, fa, fb, tb, tab);
    SISR_CHECK_LAUNCH();
    hipLaunchKernelGGL(cx_sim_kernel, dim3((unsigned)tb.blk_sim[tb.n]), block, 0, st, fa, fb, tb, (const float*)tab, S);
    SISR_CHECK_LAUNCH();
    return 0;
}

static bool cx_h_ok(float h) { return std::isfinite(h) && h > 0.f; }

extern "C" int sisr_cx_sim(const float* fa, const float* fb, int32_t B, int64_t total, int32_t n_taps, const int32_t* shapes, void* tab,
                           float* sim, void* stream) {
    if (!fa || !fb || !tab || !sim || ((uintptr_t)tab & 3) || total < 1) return SISR_E_BADARG;
    CxTable tb;
    if (int e = cx_table(B, total, n_taps, shapes, nullptr, tb)) return e;
    return cx_similarity(fa, fb, tb, (float*)tab, sim, sisr_stream(stream));
}

extern "C" int sisr_cx_fwd(const float* fa, const float* fb, int32_t B, int64_t total, int32_t n_taps, const int32_t* shapes,
                           const float* layer_w, float band_width, float weight, void* tab, void* ws, float* terms, float* cx,
                           float* loss, void* stream) {
    if (!fa || !fb || !layer_w || !tab || !ws || !cx || !loss || ((uintptr_t)tab & 3) || ((uintptr_t)ws & 15) || total < 1 ||
        !cx_h_ok(band_width))
        return SISR_E_BADARG;
    CxTable tb;
    if (int e = cx_table(B, total, n_taps, shapes, layer_w, tb)) return e;
    hipStream_t st = sisr_stream(stream);
    double* part = (double*)ws;
    float* S = (float*)((char*)ws + cx_part_bytes(tb));
    if (int e = cx_similarity(fa, fb, tb, (float*)tab, S, st)) return e;
    const dim3 block(SISR_BLOCK);
    const float inv_h = 1.f / band_width;
    hipLaunchKernelGGL(cx_row_kernel, dim3((unsigned)tb.blk_row[n_taps]), block, 0, st, (const float*)S, tb, inv_h, (float*)tab);
    SISR_CHECK_LAUNCH();
    hipLaunchKernelGGL(cx_col_kernel, dim3((unsigned)tb.blk_col[n_taps]), block, 0, st, (const float*)S, tb, inv_h, (float*)tab, part);
    SISR_CHECK_LAUNCH();
    hipLaunchKernelGGL(cx_finish_kernel, dim3(1), block, 0, st, tb, (const double*)part, (double)weight, cx, terms, loss);
    SISR_CHECK_LAUNCH();
    return 0;
}

extern "C" int sisr_cx_bwd(const float* fa, const float* fb, const void* tab, const float* cx, const float* g, int32_t B, int64_t total,
                           int32_t n_taps, const int32_t* shapes, const float* layer_w, float band_width, float weight, void* ws,
                           float* dfa, void* stream) {
    if (!fa || !fb || !layer_w || !tab || !cx || !g || !ws || !dfa || ((uintptr_t)tab & 3) || ((uintptr_t)ws & 15) || total < 1 ||
        !cx_h_ok(band_width))
        return SISR_E_BADARG;
    CxTable tb;
    if (int e = cx_table(B, total, n_taps, shapes, layer_w, tb)) return e;
    hipStream_t st = sisr_stream(stream);
    float* S = (float*)ws;
    float* dxh = S + tb.n_s;
    const float* tabf = (const float*)tab;
    const dim3 block(SISR_BLOCK);
    // S again, by the forward's own kernel from the saved mu and norms
    hipLaunchKernelGGL(cx_sim_kernel, dim3((unsigned)tb.blk_sim[n_taps]), block, 0, st, fa, fb, tb, tabf, S);
    SISR_CHECK_LAUNCH();
    hipLaunchKernelGGL(cx_bwd_row_kernel, dim3((unsigned)tb.blk_row[n_taps]), block, 0, st, S, tb, 1.f / band_width, tabf, cx, g,
                       (double)weight);
    SISR_CHECK_LAUNCH();
    hipLaunchKernelGGL(cx_bwd_mm_kernel, dim3((unsigned)tb.blk_mm[n_taps]), block, 0, st, fb, (const float*)S, tb, tabf, dxh);
    SISR_CHECK_LAUNCH();
    hipLaunchKernelGGL(cx_bwd_proj_kernel, dim3((unsigned)tb.blk_pt[n_taps]), block, 0, st, fa, (const float*)dxh, tb, tabf, dfa);
    SISR_CHECK_LAUNCH();
    return 0;
}
