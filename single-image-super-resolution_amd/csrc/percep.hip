// percep.hip -- the multi-tap perceptual loss of the ESRGAN / Real-ESRGAN family (BasicSR's PerceptualLoss) with its optional style
// term on the Gram matrices of the same taps, forward and backward.  fa, fb: fp32 [B][total], the output
// layout of MaskedVGG.forward: tap l is columns [off_l, off_l + C_l P_l) of every row in NCHW order, F_x,l[n] that slice as C_l x P_l:
//   T_l = crit(fa_l, fb_l)            G_x,l[n] = F_x,l[n] F_x,l[n]^T / (C_l P_l)            S_l = crit(G_a,l, G_b,l) over B C_l^2 elements
//   crit: L1 mean |d|, L2 mean d^2, FRO sqrt(sum d^2) over the whole batch tensor of the tap
//   perceptual = pw sum_l w_l T_l,   style = sw sum_l w_l S_l
//   with D_l[n] = dS_l / dG_a,l[n] (symmetric):  dstyle / dF_a = (2 / (C P)) D F_a,   dstyle / dF_b = -(2 / (C P)) D F_b
// Launches (none depends on B; a term whose weight is 0 launches nothing):
//   percep_gram_kernel     style: every (tap, input, sample, 32 x 32 tile on or above the diagonal, split of P) is one workgroup of a
//                          table walk.  Chunks of PG_KC columns of the tile's 32 + 32 channel rows go from memory (16-byte loads
//                          along P where the tap's offset allows, else 4-byte ones; the next chunk's loads are in flight while this
//                          one is multiplied) into LDS as [p][channel] with pitch PG_PITCH = 64 + 32, the pitch scheme of
//                          fc_wgrad_rows_kernel: both operands of v_mfma_f32_32x32x2_f32 want lanes along the channel, which is
//                          stride P in memory.  Ragged tiles and an odd K tail are zeros in LDS.  The four waves take a quarter of
//                          the chunk's K steps each and meet in LDS in wave order; the tile and its mirror are stored from the same
//                          sums into the workgroup's partial [C][C] of the workspace.  No atomics.
//   percep_finish_kernel   style: G = (partials added in split order) / (C P) for both inputs, d = G_a - G_b, the criterion's terms
//                          as one double partial per workgroup, and D (l1: sign(d) / (B C^2), l2: 2 d / (B C^2), fro: d; the fro
//                          norm divides in the backward) when a gradient is wanted.  The Gram-only entry runs it to store G.
//   percep_feature_kernel  perceptual: one table-driven pass over (fa, fb), a double partial per workgroup.
//   percep_terms_kernel    one workgroup: per tap the partials of both terms in a fixed order in double, the tables, the two scalars.
//   percep_bwd_kernel      D F with K = C on the same instruction, operands straight from memory (D is symmetric: lanes along a
//                          row of it; F: lanes along p), a wave owns 32 rows x 128 columns (four accumulators); the feature term's
//                          derivative is added in the epilogue; every gradient element is stored once.
// Every sum has a fixed order: the same bits on every call, nothing is read back by the host, the launches can be captured.
#include "sisr_dev.h"

#include <algorithm>
#include <cmath>

#ifndef PG_KC
#define PG_KC 64                      // columns of P per staged chunk (24 KB of LDS; 128 was measured 10 % slower: DESIGN.md section 29)
#endif
#define PG_U (PG_KC / 32)              // 16-byte pieces of a thread per chunk and half: 32 rows x PG_KC / 4 pieces over 256 threads
#define PG_PITCH 96                   // LDS pitch of a staged column: 32 + 32 channel slots + 32
#define PG_TARGET_WG 1024             // workgroups of a tap the split along P aims at
#define PG_MAX_SPLIT 64
#define PF_ELEMS 1024                 // Gram elements of a finish workgroup
#define PE_CHUNK 16384                // feature elements of a feature-term workgroup
#define PB_ACC 4                      // accumulators (32 columns each) of a backward wave
#define PB_COLS (4 * 32 * PB_ACC)     // columns of a backward workgroup
static_assert(SISR_BLOCK == 256 && PG_KC % 64 == 0 && 4 * 32 * 33 <= PG_KC * PG_PITCH, "the staging map is written for 256 threads; the waves meet inside the staged chunk");

struct PcTap {
    int C, P, T, ntp;                 // T = tiles of 32 channels, ntp = T (T + 1) / 2
    int S, cps;                       // splits along P, chunks of PG_KC per split
    int vec;                          // bit 0: 16-byte loads along a feature row; bit 1: along a channel row
    float w;
    int64_t off;                      // first column of the tap
    int64_t part, d;                  // floats before the tap in the Gram partials of ONE input / in D and the Gram output
};
struct PcTable {
    int n, B;
    int64_t total;
    int64_t part_x;                   // floats of one input's Gram partials
    int blk_gram[SISR_PERCEP_MAX_TAPS + 1], blk_fin[SISR_PERCEP_MAX_TAPS + 1], blk_feat[SISR_PERCEP_MAX_TAPS + 1],
        blk_bwd[SISR_PERCEP_MAX_TAPS + 1];      // first workgroup of each tap in the four walks (gram and bwd: per input)
    PcTap t[SISR_PERCEP_MAX_TAPS];
};
struct PcWs {
    double* feat;                     // [blk_feat[n]]
    double* sty;                      // [blk_fin[n]]
    float* part;                      // [2][part_x]
    int64_t feat_bytes, bytes;
};

__device__ __forceinline__ int pc_tap_of(const int* blk0, int n, int b) {
    int l = 0;
    while (l + 1 < n && b >= blk0[l + 1]) ++l;
    return l;
}

// ---- Gram partials: blockIdx.x = x * blk_gram[n] + (blk_gram[l] + ((n * ntp + tp) * S + s)) ------------------------------------------
__global__ void __launch_bounds__(SISR_BLOCK) percep_gram_kernel(const float* __restrict__ fa, const float* __restrict__ fb, PcTable tb,
                                                                 float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float stage[PG_KC * PG_PITCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, kk = lane >> 5;
    const int per_x = tb.blk_gram[tb.n];
    const int x = (int)blockIdx.x / per_x, bx = (int)blockIdx.x - x * per_x;
    const int l = pc_tap_of(tb.blk_gram, tb.n, bx);
    const PcTap t = tb.t[l];
    int r = bx - tb.blk_gram[l];
    const int s = r % t.S;
    r /= t.S;
    int tp = r % t.ntp;
    const int n = r / t.ntp;
    int ti = 0;
    while (tp >= t.T - ti) { tp -= t.T - ti; ++ti; }
    const int tj = ti + tp;
    const int i0 = ti * 32, j0 = tj * 32, halves = ti == tj ? 1 : 2;
    const float* __restrict__ F = (x ? fb : fa) + (int64_t)n * tb.total + t.off;
    const int nchunks = (t.P + PG_KC - 1) / PG_KC;
    const int c0 = s * t.cps, c1 = min(c0 + t.cps, nchunks);
    const bool vec = (t.vec & 2) != 0;

    // this thread's pieces of a chunk: channel row tid & 31 of half u / PG_U, columns 4 q .. 4 q + 3 with q = (tid >> 5) + 8 (u % PG_U): the two
    // halves of a wave hold the 32 channels of one q each, so a column's 32 stores fall on 32 banks
    const int sc = tid & 31, sq = tid >> 5;
    f32x4 v[2 * PG_U];
    auto fetch = [&](int chunk) {
#pragma unroll
        for (int u = 0; u < 2 * PG_U; ++u) {
            v[u] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (u < PG_U * halves) {
                const int row = (u < PG_U ? i0 : j0) + sc;
                const int p = chunk * PG_KC + 4 * (sq + 8 * (u % PG_U));
                if (row < t.C && p < t.P) {
                    const float* src = F + (int64_t)row * t.P + p;
                    if (vec) {
                        v[u] = *reinterpret_cast<const f32x4*>(src);           // P % 4 == 0: the piece is inside the row
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (p + j < t.P) v[u][j] = src[j];
                    }
                }
            }
        }
    };
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    if (c0 < c1) fetch(c0);
    for (int chunk = c0; chunk < c1; ++chunk) {
        if (chunk > c0) __syncthreads();                           // the previous chunk has been multiplied
#pragma unroll
        for (int u = 0; u < 2 * PG_U; ++u) {
            if (u < PG_U * halves) {
                const int q = sq + 8 * (u % PG_U);
#pragma unroll
                for (int j = 0; j < 4; ++j) stage[(4 * q + j) * PG_PITCH + (u / PG_U) * 32 + sc] = v[u][j];
            }
        }
        __syncthreads();
        if (chunk + 1 < c1) fetch(chunk + 1);                      // in flight during the products
        // steps of two columns; a chunk past the end of P holds zeros, whole steps of them are skipped
        const int cols = min(PG_KC, t.P - chunk * PG_KC), steps = (cols + 1) >> 1;
        const int s0 = wave * (PG_KC / 8), s1 = min(s0 + PG_KC / 8, steps);
        const float* ap = stage + kk * PG_PITCH + l31;
        const float* bp = ap + (halves - 1) * 32;
        for (int st = s0; st < s1; ++st) acc = mfma32(ap[2 * st * PG_PITCH], bp[2 * st * PG_PITCH], acc);
    }
    // the four waves meet in LDS (pitch 33), added in wave order; acc[reg]: row mfma_row(reg, lane), column l31
    __syncthreads();
    float* red = stage;
#pragma unroll
    for (int i = 0; i < 16; ++i) red[wave * (32 * 33) + mfma_row(i, lane) * 33 + l31] = acc[i];
    __syncthreads();
    float* out = part + (int64_t)x * tb.part_x + t.part + ((int64_t)n * t.S + s) * t.C * t.C;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int e = tid + SISR_BLOCK * u, rr = e >> 5, cc = e & 31;
        if (i0 + rr < t.C && j0 + cc < t.C) {
            const int a = rr * 33 + cc;
            out[(int64_t)(i0 + rr) * t.C + j0 + cc] = ((red[a] + red[a + 32 * 33]) + red[a + 2 * 32 * 33]) + red[a + 3 * 32 * 33];
        }
        if (halves == 2 && j0 + rr < t.C && i0 + cc < t.C) {      // the mirror: the same four values in the same order
            const int a = cc * 33 + rr;
            out[(int64_t)(j0 + rr) * t.C + i0 + cc] = ((red[a] + red[a + 32 * 33]) + red[a + 2 * 32 * 33]) + red[a + 3 * 32 * 33];
        }
    }
}

// G[e] of one sample: the partials of its splits added in split order, over C P
__device__ __forceinline__ float pc_gram_value(const float* __restrict__ part, int S, int64_t cc, int64_t e, float cp) {
    float g = part[e];
    for (int s = 1; s < S; ++s) g += part[(int64_t)s * cc + e];
    return g / cp;
}

// ---- finish: blockIdx.x = blk_fin[l] + block of PF_ELEMS elements of the tap's [B][C][C].  LOSS: the criterion over (G_a, G_b);
// else G of input 0 -> gram ----------------------------------------------------------------------------------------------------------
template <bool LOSS>
__global__ void __launch_bounds__(SISR_BLOCK) percep_finish_kernel(PcTable tb, const float* __restrict__ part, int crit,
                                                                   double* __restrict__ sty, float* __restrict__ dmat,
                                                                   float* __restrict__ gram) {
    const int l = pc_tap_of(tb.blk_fin, tb.n, (int)blockIdx.x);
    const PcTap t = tb.t[l];
    const int64_t cc = (int64_t)t.C * t.C, count = tb.B * cc;
    const int64_t e0 = (int64_t)((int)blockIdx.x - tb.blk_fin[l]) * PF_ELEMS;
    const float cp = (float)((int64_t)t.C * t.P);
    const double inv = 1.0 / (double)count;
    double sum[1] = {0.0};
#pragma unroll
    for (int u = 0; u < PF_ELEMS / SISR_BLOCK; ++u) {
        const int64_t i = e0 + threadIdx.x + SISR_BLOCK * u;
        if (i < count) {
            const int64_t n = i / cc, e = i - n * cc;
            const float* pa = part + t.part + n * t.S * cc;
            const float ga = pc_gram_value(pa, t.S, cc, e, cp);
            if (!LOSS) {
                gram[t.d + i] = ga;
            } else {
                const float d = ga - pc_gram_value(pa + tb.part_x, t.S, cc, e, cp);
                float dv;
                if (crit == SISR_PERCEP_L1) {
                    sum[0] += (double)fabsf(d);
                    dv = d > 0.f ? (float)inv : (d < 0.f ? -(float)inv : 0.f);
                } else {
                    sum[0] += (double)d * (double)d;
                    dv = crit == SISR_PERCEP_L2 ? (float)(2.0 * (double)d * inv) : d;
                }
                if (dmat) dmat[t.d + i] = dv;
            }
        }
    }
    if (LOSS) {
        block_partial_sum<double, 1>(sum);
        if (threadIdx.x == 0) sty[blockIdx.x] = sum[0];
    }
}

// ---- feature term: blockIdx.x = blk_feat[l] + n * chunks + chunk of PE_CHUNK elements of the sample's slice ------------------------------
__global__ void __launch_bounds__(SISR_BLOCK) percep_feature_kernel(const float* __restrict__ fa, const float* __restrict__ fb,
                                                                    PcTable tb, int crit, double* __restrict__ feat) {
    const int l = pc_tap_of(tb.blk_feat, tb.n, (int)blockIdx.x);
    const PcTap t = tb.t[l];
    const int64_t cp = (int64_t)t.C * t.P;
    const int chunks = (int)((cp + PE_CHUNK - 1) / PE_CHUNK);
    const int r = (int)blockIdx.x - tb.blk_feat[l], n = r / chunks, ck = r - n * chunks;
    const int64_t base = (int64_t)n * tb.total + t.off + (int64_t)ck * PE_CHUNK;
    const int len = (int)min((int64_t)PE_CHUNK, cp - (int64_t)ck * PE_CHUNK);
    const float* __restrict__ a = fa + base;
    const float* __restrict__ b = fb + base;
    const bool l1 = crit == SISR_PERCEP_L1;
    double sum[1] = {0.0};
    int done = 0;
    if (t.vec & 1) {                                               // 16-byte pieces; the last chunk's <= 3 elements behind them below
        const int len4 = len >> 2;
        for (int i = threadIdx.x; i < len4; i += SISR_BLOCK) {
            const f32x4 x = reinterpret_cast<const f32x4*>(a)[i], y = reinterpret_cast<const f32x4*>(b)[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float d = x[j] - y[j];
                sum[0] += l1 ? (double)fabsf(d) : (double)d * (double)d;
            }
        }
        done = 4 * len4;
    }
    for (int i = done + threadIdx.x; i < len; i += SISR_BLOCK) {
        const float d = a[i] - b[i];
        sum[0] += l1 ? (double)fabsf(d) : (double)d * (double)d;
    }
    block_partial_sum<double, 1>(sum);
    if (threadIdx.x == 0) feat[blockIdx.x] = sum[0];
}

// ---- the tables and the scalars: one workgroup -------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SISR_BLOCK) percep_terms_kernel(PcTable tb, int crit, const double* __restrict__ feat,
                                                                  const double* __restrict__ sty, double pw, double sw,
                                                                  float* __restrict__ terms_p, float* __restrict__ terms_s,
                                                                  float* __restrict__ perceptual, float* __restrict__ style) {
    double tot_p = 0.0, tot_s = 0.0;
    for (int l = 0; l < tb.n; ++l) {
        const PcTap t = tb.t[l];
        if (perceptual) {
            const double* p = feat + tb.blk_feat[l];
            double s[1];
            fold_partials_double<1>(tb.blk_feat[l + 1] - tb.blk_feat[l], s, [&](int64_t i, double (&acc)[1]) { acc[0] += p[i]; });
            const double v = crit == SISR_PERCEP_FRO ? sqrt(s[0]) : s[0] / ((double)tb.B * t.C * t.P);
            if (threadIdx.x == 0 && terms_p) terms_p[l] = (float)v;
            tot_p += (double)t.w * v;
            __syncthreads();                                       // the fold's LDS is free again
        }
        if (style) {
            const double* p = sty + tb.blk_fin[l];
            double s[1];
            fold_partials_double<1>(tb.blk_fin[l + 1] - tb.blk_fin[l], s, [&](int64_t i, double (&acc)[1]) { acc[0] += p[i]; });
            const double v = crit == SISR_PERCEP_FRO ? sqrt(s[0]) : s[0] / ((double)tb.B * t.C * t.C);
            if (threadIdx.x == 0 && terms_s) terms_s[l] = (float)v;
            tot_s += (double)t.w * v;
            __syncthreads();
        }
    }
    if (threadIdx.x == 0) {
        if (perceptual) perceptual[0] = (float)(pw * tot_p);
        if (style) style[0] = (float)(sw * tot_s);
    }
}

// ---- backward: blockIdx.x = xi * blk_bwd[n] + (blk_bwd[l] + ((n * blocks of PB_COLS columns + pb) * T + ti)); a wave owns rows
// 32 ti .. + 31 and 32 PB_ACC columns.  xi walks the wanted gradients: both (dfa then dfb) or the one that is not null ------------------
__global__ void __launch_bounds__(SISR_BLOCK) percep_bwd_kernel(const float* __restrict__ fa, const float* __restrict__ fb,
                                                                const float* __restrict__ dmat, const float* __restrict__ terms_p,
                                                                const float* __restrict__ terms_s, const float* __restrict__ g_p,
                                                                const float* __restrict__ g_s, PcTable tb, double pw, double sw,
                                                                int crit, float* __restrict__ dfa, float* __restrict__ dfb) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, kk = lane >> 5;
    const int per_x = tb.blk_bwd[tb.n];
    const int xi = (int)blockIdx.x / per_x, bx = (int)blockIdx.x - xi * per_x;
    const int x = dfa ? xi : 1;
    const int l = pc_tap_of(tb.blk_bwd, tb.n, bx);
    const PcTap t = tb.t[l];
    int r = bx - tb.blk_bwd[l];
    const int ti = r % t.T;
    r /= t.T;
    const int npb = (t.P + PB_COLS - 1) / PB_COLS;
    const int pb = r % npb, n = r / npb;
    const int i0 = ti * 32, p0 = pb * PB_COLS + wave * (32 * PB_ACC);
    if (p0 >= t.P) return;
    const int64_t row0 = (int64_t)n * tb.total + t.off;
    const float* __restrict__ F = (x ? fb : fa) + row0;
    float* __restrict__ O = (x ? dfb : dfa) + row0;
    const bool with_style = g_s != nullptr, with_feat = g_p != nullptr;
    const double cpd = (double)t.C * (double)t.P;

    f32x16 acc[PB_ACC];
#pragma unroll
    for (int a = 0; a < PB_ACC; ++a)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[a][i] = 0.f;
    float cs = 0.f, cf = 0.f;
    if (with_style) {
        double c = 2.0 * (double)g_s[0] * sw * (double)t.w / cpd;
        if (crit == SISR_PERCEP_FRO) {
            const double nrm = (double)terms_s[l];
            c = nrm == 0.0 ? 0.0 : c / nrm;                         // (a NaN norm stays a NaN)
        }
        cs = (float)(x ? -c : c);
        const float* __restrict__ D = dmat + t.d + (int64_t)n * t.C * t.C;
        const bool iok = i0 + l31 < t.C;
        for (int k = 0; k < t.C; k += 2) {
            const int kr = k + kk;
            const bool ok = kr < t.C;
            const float a = (ok && iok) ? D[(int64_t)kr * t.C + i0 + l31] : 0.f;       // D[i][kr] == D[kr][i]
            float b[PB_ACC];
#pragma unroll
            for (int u = 0; u < PB_ACC; ++u) {
                const int col = p0 + 32 * u + l31;
                b[u] = (ok && col < t.P) ? F[(int64_t)kr * t.P + col] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < PB_ACC; ++u) acc[u] = mfma32(a, b[u], acc[u]);
        }
    }
    if (with_feat) {
        double c = (double)g_p[0] * pw * (double)t.w;
        if (crit == SISR_PERCEP_FRO) {
            const double nrm = (double)terms_p[l];
            c = nrm == 0.0 ? 0.0 : c / nrm;
        } else {
            c = (crit == SISR_PERCEP_L2 ? 2.0 : 1.0) * c / ((double)tb.B * cpd);
        }
        cf = (float)(x ? -c : c);
    }
    const float* __restrict__ A = fa + row0;
    const float* __restrict__ Bf = fb + row0;
#pragma unroll
    for (int u = 0; u < PB_ACC; ++u) {
        const int col = p0 + 32 * u + l31;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int row = i0 + mfma_row(i, lane);
            if (row < t.C && col < t.P) {
                const int64_t idx = (int64_t)row * t.P + col;
                float val = with_style ? cs * acc[u][i] : 0.f;
                if (with_feat) {
                    const float d = A[idx] - Bf[idx];
                    const float sd = crit == SISR_PERCEP_L1 ? (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f)) : d;
                    val = fmaf(cf, sd, val);
                }
                O[idx] = val;
            }
        }
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------------------------
static bool pc_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// the table of a call -> 0 or a status code.  `total`: < 0 skips the sum check (the size query)
static int percep_table(int32_t B, int64_t total, int32_t n_taps, const int32_t* shapes, const float* layer_w, PcTable& tb) {
    if (!shapes || B < 1 || n_taps < 1 || n_taps > SISR_PERCEP_MAX_TAPS) return SISR_E_BADARG;
    tb.n = n_taps;
    tb.B = B;
    tb.total = total;
    int64_t off = 0, part = 0, d = 0, bg = 0, bf = 0, be = 0, bb = 0;
    for (int l = 0; l < n_taps; ++l) {
        const int64_t C = shapes[3 * l], H = shapes[3 * l + 1], W = shapes[3 * l + 2];
        if (C < 1 || H < 1 || W < 1) return SISR_E_BADARG;
        if (H * W > INT32_MAX / C) return SISR_E_TOOBIG;
        PcTap& t = tb.t[l];
        t.C = (int)C;
        t.P = (int)(H * W);
        t.T = (int)((C + 31) / 32);
        t.ntp = t.T * (t.T + 1) / 2;
        const int64_t nchunks = (t.P + PG_KC - 1) / PG_KC;
        int64_t S = (PG_TARGET_WG + (int64_t)B * t.ntp - 1) / ((int64_t)B * t.ntp);      // the same for one input and for two
        S = std::min<int64_t>(std::min<int64_t>(S, PG_MAX_SPLIT), nchunks);
        t.cps = (int)((nchunks + S - 1) / S);
        t.S = (int)((nchunks + t.cps - 1) / t.cps);                                      // no split without a chunk
        t.vec = 0;
        t.w = layer_w ? layer_w[l] : 1.f;
        t.off = off;
        t.part = part;
        t.d = d;
        tb.blk_gram[l] = (int)bg;
        tb.blk_fin[l] = (int)bf;
        tb.blk_feat[l] = (int)be;
        tb.blk_bwd[l] = (int)bb;
        off += C * t.P;
        part += (int64_t)B * t.S * C * C;
        d += (int64_t)B * C * C;
        bg += (int64_t)B * t.ntp * t.S;
        bf += ((int64_t)B * C * C + PF_ELEMS - 1) / PF_ELEMS;
        be += (int64_t)B * ((C * t.P + PE_CHUNK - 1) / PE_CHUNK);
        bb += (int64_t)B * ((t.P + PB_COLS - 1) / PB_COLS) * t.T;
        if (off > ((int64_t)1 << 40) || part > ((int64_t)1 << 40) || std::max(std::max(bg, bf), std::max(be, bb)) > INT32_MAX / 2)
            return SISR_E_TOOBIG;
    }
    if (total >= 0 && off != total) return SISR_E_BADARG;
    tb.part_x = part;
    tb.blk_gram[n_taps] = (int)bg;
    tb.blk_fin[n_taps] = (int)bf;
    tb.blk_feat[n_taps] = (int)be;
    tb.blk_bwd[n_taps] = (int)bb;
    return 0;
}

// which loads of a tap may be 16 bytes wide: every row of every pointer starts on a 16-byte line
static void percep_vec(PcTable& tb, const void* p0, const void* p1) {
    const bool base = pc_aligned16(p0) && (!p1 || pc_aligned16(p1)) && tb.total % 4 == 0;
    for (int l = 0; l < tb.n; ++l) {
        PcTap& t = tb.t[l];
        const bool row = base && t.off % 4 == 0;
        t.vec = (row ? 1 : 0) | (row && t.P % 4 == 0 ? 2 : 0);
    }
}

// the workspace: the feature term's partials, the style term's (doubles), the Gram partials of both inputs (floats)
static void percep_ws(const PcTable& tb, bool with_feature, bool with_style, void* ws, PcWs& w) {
    const int64_t nf = with_feature ? ((int64_t)tb.blk_feat[tb.n] + 1) & ~(int64_t)1 : 0;      // even: 16-byte lines
    const int64_t ns = with_style ? ((int64_t)tb.blk_fin[tb.n] + 1) & ~(int64_t)1 : 0;
    w.feat = (double*)ws;
    w.sty = w.feat + nf;
    w.part = (float*)(w.sty + ns);
    w.feat_bytes = 8 * nf;
    w.bytes = 8 * (nf + ns) + (with_style ? 4 * 2 * tb.part_x : 0);
}

extern "C" int64_t sisr_percep_ws_bytes(int32_t B, int32_t n_taps, const int32_t* shapes, int32_t with_feature, int32_t with_style) {
    PcTable tb;
    if (int e = percep_table(B, -1, n_taps, shapes, nullptr, tb)) return e;
    PcWs w;
    percep_ws(tb, with_feature != 0, with_style != 0, nullptr, w);
    return w.bytes;
}

extern "C" int sisr_percep_gram(const float* f, int32_t B, int64_t total, int32_t n_taps, const int32_t* shapes, void* ws, float* gram,
                                void* stream) {
    if (!f || !ws || !gram || ((uintptr_t)ws & 15) || total < 1) return SISR_E_BADARG;
    PcTable tb;
    if (int e = percep_table(B, total, n_taps, shapes, nullptr, tb)) return e;
    percep_vec(tb, f, nullptr);
    PcWs w;
    percep_ws(tb, false, true, ws, w);
    hipStream_t st = sisr_stream(stream);
    hipLaunchKernelGGL(percep_gram_kernel, dim3((unsigned)tb.blk_gram[n_taps]), dim3(SISR_BLOCK), 0, st, f, f, tb, w.part);
    SISR_CHECK_LAUNCH();
    hipLaunchKernelGGL(percep_finish_kernel<false>, dim3((unsigned)tb.blk_fin[n_taps]), dim3(SISR_BLOCK), 0, st, tb,
                       (const float*)w.part, 0, (double*)nullptr, (float*)nullptr, gram);
    SISR_CHECK_LAUNCH();
    return 0;
}

static bool percep_crit_ok(int32_t crit) { return crit == SISR_PERCEP_L1 || crit == SISR_PERCEP_L2 || crit == SISR_PERCEP_FRO; }

extern "C" int sisr_percep_fwd(const float* fa, const float* fb, int32_t B, int64_t total, int32_t n_taps, const int32_t* shapes,
                               const float* layer_w, float perceptual_weight, float style_weight, int32_t crit, void* ws,
                               float* terms_p, float* terms_s, float* perceptual, float* style, float* dmat, void* stream) {
    if (!fa || !fb || !ws || !layer_w || ((uintptr_t)ws & 15) || total < 1 || !percep_crit_ok(crit)) return SISR_E_BADARG;
    const bool with_p = perceptual_weight != 0.f, with_s = style_weight != 0.f;
    if ((with_p && !perceptual) || (with_s && !style) || (!with_p && !with_s)) return SISR_E_BADARG;
    PcTable tb;
    if (int e = percep_table(B, total, n_taps, shapes, layer_w, tb)) return e;
    percep_vec(tb, fa, fb);
    PcWs w;
    percep_ws(tb, with_p, with_s, ws, w);
    hipStream_t st = sisr_stream(stream);
    const dim3 block(SISR_BLOCK);
    if (with_s) {
        hipLaunchKernelGGL(percep_gram_kernel, dim3(2u * (unsigned)tb.blk_gram[n_taps]), block, 0, st, fa, fb, tb, w.part);
        SISR_CHECK_LAUNCH();
        hipLaunchKernelGGL(percep_finish_kernel<true>, dim3((unsigned)tb.blk_fin[n_taps]), block, 0, st, tb, (const float*)w.part,
                           (int)crit, w.sty, dmat, (float*)nullptr);
        SISR_CHECK_LAUNCH();
    }
    if (with_p) {
        hipLaunchKernelGGL(percep_feature_kernel, dim3((unsigned)tb.blk_feat[n_taps]), block, 0, st, fa, fb, tb, (int)crit, w.feat);
        SISR_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(percep_terms_kernel, dim3(1), block, 0, st, tb, (int)crit, (const double*)w.feat, (const double*)w.sty,
                       (double)perceptual_weight, (double)style_weight, with_p ? terms_p : nullptr, with_s ? terms_s : nullptr,
                       with_p ? perceptual : nullptr, with_s ? style : nullptr);
    SISR_CHECK_LAUNCH();
    return 0;
}

extern "C" int sisr_percep_bwd(const float* fa, const float* fb, const float* dmat, const float* terms_p, const float* terms_s,
                               const float* g_perceptual, const float* g_style, int32_t B, int64_t total, int32_t n_taps,
                               const int32_t* shapes, const float* layer_w, float perceptual_weight, float style_weight, int32_t crit,
                               float* dfa, float* dfb, void* stream) {
    if (!fa || !fb || !layer_w || (!dfa && !dfb) || total < 1 || !percep_crit_ok(crit)) return SISR_E_BADARG;
    const bool with_p = perceptual_weight != 0.f, with_s = style_weight != 0.f;
    if ((!with_p && !with_s) || (with_p && !g_perceptual) || (with_s && (!g_style || !dmat))) return SISR_E_BADARG;
    if (crit == SISR_PERCEP_FRO && ((with_p && !terms_p) || (with_s && !terms_s))) return SISR_E_BADARG;
    PcTable tb;
    if (int e = percep_table(B, total, n_taps, shapes, layer_w, tb)) return e;
    const unsigned nx = dfa && dfb ? 2u : 1u;
    hipLaunchKernelGGL(percep_bwd_kernel, dim3(nx * (unsigned)tb.blk_bwd[n_taps]), dim3(SISR_BLOCK), 0, sisr_stream(stream), fa, fb,
                       dmat, terms_p, terms_s, with_p ? g_perceptual : nullptr, with_s ? g_style : nullptr, tb,
                       (double)perceptual_weight, (double)style_weight, (int)crit, dfa, dfb);
    SISR_CHECK_LAUNCH();
    return 0;
}
