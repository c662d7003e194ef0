// freq_loss.hip -- the frequency-domain training loss of two fp32 NCHW batches, forward and backward, entirely on the device.
// On the view of sisr_ssim.h (`crop` pixels stripped from every side, BT.601 luma for C == 3 with `luma`: [N][C'][H'][W']):
//   d = view(a) - view(b),   D[kh, kw] = sum_{y,x} d[y, x] exp(-2 pi i (kh y / H' + kw x / W')),   Wh = W' / 2 + 1
//   L1 / Charbonnier: loss[n] = mean over (C', kh < H', kw < Wh, {Re, Im}) of rho(.),   rho(z) = |z| / sqrt(z^2 + eps^2)
//                     (BasicSR's FFTLoss: the half spectrum as rfft2 returns it, unnormalised, no Hermitian doubling)
//   focal:            loss[n] = mean_{C', kh, kw} w dist over the FULL ortho-normalised spectrum, dist = |D|^2 / (H' W'),
//                     w = dist^(alpha/2) / max_{kh,kw} dist^(alpha/2) per (n, plane), a constant for the gradient; in closed form
//                     sum_p sum_{k in half} h_k |D_k|^(2+alpha) / (max_p|D|^alpha (H' W')^2 C'),  h_k = 1 for kw = 0 and (W' even)
//                     kw = W' / 2, otherwise 2.  A plane with a == b: loss 0, gradient 0.
// The transform is linear, so ONE transform of d serves both images.  It is a direct separable DFT (any side 1 .. 256, no
// butterflies): every workgroup builds cos / sin(2 pi j / N), j < N, of its axis in LDS from sincospi(2 j / N) in double (exact 0 / +-1 at
// j = 0, N/4, N/2, 3N/4, so Im D of the structurally real bins is exactly 0 and the L1 gradient there is sign(0) = 0) and indexes it
// with (k t) mod N carried incrementally -- an angle is never formed as a float product.
//
// All four transform passes share one scheme.  A workgroup owns FQ_LINES = 8 lines (rows for the passes along W, kw columns for
// the passes along H), staged once in LDS as [t][line]; a thread owns ONE output index k and FQ_PER = 4 lines, lanes on consecutive
// k.  Per step t a thread gathers one twiddle (8 bytes) and reads its 4 line values with one or two 16-byte LDS reads that are the
// same address for (nearly) every lane of the wave -- a broadcast -- for 8 (real) or 16 (complex) fused multiply-adds.  The block
// size follows the work: (outputs per line) x 2 groups of 4 lines, rounded up to whole waves, at most 256 -- 8 lines and not 16
// per workgroup because the grids are small (16 x 3 planes): twice the workgroups of half the length spread evenly over 256 CUs
// where 336 or 576 long ones left most CUs idle in the last round.
// The three passes whose output runs over a FULL axis (both column passes, the row inverse) give a thread the output pair
// (k, N - k): the twiddles of N - k are the conjugates of k's, so the same products serve both outputs and the arithmetic and the
// LDS reads per output halve (fq_column_dft_pair).  The forward row pass only produces kw <= W' / 2 and has no partner to share with.
//
// Forward, three launches: (1) rows: d staged with crop offset, luma and the subtraction applied on load -> the half spectrum along
// W of every row, `work` [N][C'][H'][Wh][2]; (2) columns: the complex DFT along H, rho or h |D|^(2+alpha) formed in registers, D
// stored to `spec` when a gradient will be needed, one partial (sum, max |D|^2) per workgroup; (3) finish: one workgroup per image
// folds the partials in a fixed order in double, focal divides by the plane's max^alpha and stores the plane maxima.
// Backward, two launches in gather form: (1) columns: G = g[n] coef rho'(D) (focal: g[n] 2 h_k w_k D / ((H' W')^2 C')) formed on load
// from `spec`, transformed along H with conjugate twiddles -> `work`; (2) rows: grad_d[y, x] = sum_kw Re(T[y, kw] e^{+i theta}),
// the view's transpose applied (luma weights to three channels, sign -1 for b), da / db written directly over the WHOLE image, so
// the cropped border gets exact zeros.  The inputs are not needed by the backward: saved are D (about one input's size) and the
// plane maxima.  No atomics, plain vector stores, fixed-order sums: the same bits every call, capturable.
#include "sisr_dev.h"

#include <cmath>

#define FQ_LINES 8
#define FQ_PER 4
#define FQ_GROUPS (FQ_LINES / FQ_PER)
#define FQ_RPAD (FQ_LINES + 4)          // floats per x of the staged real rows (16-byte aligned, stores spread over banks)
#define FQ_CROW (2 * FQ_LINES)          // floats per step of staged complex lines, column passes (stores: lanes on consecutive lines)
#define FQ_CPAD (2 * FQ_LINES + 4)      // ... row inverse (stores: lanes on consecutive kw, so the step stride must not be a power of two)
#define FQ_MAX_WH (SISR_FREQ_MAX_SIDE / 2 + 1)

struct FreqGeom {
    int C, H, W, crop, luma;
    int Hv, Wv, Wh;                     // the view, and the half spectrum's width
    int planes;                         // C'
    int rblocks, cblocks, iblocks;      // blocks of 8: view rows, kw columns, rows of the whole image
};

static int freq_geom(int N, int C, int H, int W, int crop, int luma, FreqGeom& g) {
    if (N <= 0 || crop < 0 || H <= 0 || W <= 0) return SISR_E_BADARG;
    if (C != 1 && C != 3) return SISR_E_UNSUPPORTED;
    const int64_t hv = (int64_t)H - 2 * (int64_t)crop, wv = (int64_t)W - 2 * (int64_t)crop;
    if (hv < 1 || wv < 1 || hv > SISR_FREQ_MAX_SIDE || wv > SISR_FREQ_MAX_SIDE) return SISR_E_BADARG;
    g.C = C; g.H = H; g.W = W; g.crop = crop;
    g.luma = (luma != 0 && C == 3) ? 1 : 0;
    g.Hv = (int)hv; g.Wv = (int)wv; g.Wh = g.Wv / 2 + 1;
    g.planes = g.luma ? 1 : C;
    g.rblocks = (g.Hv + FQ_LINES - 1) / FQ_LINES;
    g.cblocks = (g.Wh + FQ_LINES - 1) / FQ_LINES;
    g.iblocks = (H + FQ_LINES - 1) / FQ_LINES;
    return 0;
}

static int64_t freq_spec_floats(int N, const FreqGeom& g) { return 2 * (int64_t)N * g.planes * g.Hv * g.Wh; }

// one pixel of the view; off: the element of the first plane
__device__ __forceinline__ float fq_load(const float* __restrict__ p, int64_t off, int64_t plane_elems, int luma) {
    return luma ? fmaf(0.114f, p[off + 2 * plane_elems], fmaf(0.587f, p[off + plane_elems], 0.299f * p[off])) : p[off];
}

// tw[j] = (cos, sin)(2 pi j / n), j < n <= 256, rounded once from double; ends with a barrier
__device__ __forceinline__ void fq_twiddles(float2* tw, int n) {
    for (int j = threadIdx.x; j < n; j += blockDim.x) {
        double s, c;
        sincospi(2.0 * (double)j / (double)n, &s, &c);
        tw[j] = make_float2((float)c, (float)s);
    }
    __syncthreads();
}

// The complex DFT along H of 8 staged columns, st [Hv][8][2], for the output pair (k, Hv - k) of the 4 columns of group grp.
// The twiddles of Hv - k are the conjugates of k's, so the four real sums A = sum vr cos, B = sum vi sin, C = sum vi cos,
// E = sum vr sin serve both outputs: 4 fused multiply-adds per value and step for two outputs instead of 4 for one.
//   SIGN < 0 (e^{-i theta}):  out(k) = (A + B, C - E),  out(Hv - k) = (A - B, C + E);   SIGN > 0: the two exchanged.
// A bin whose twiddles are all 0 / +-1 keeps its exact zeros: B and E are then sums of exact zeros.
template <int SIGN>
__device__ __forceinline__ void fq_column_dft_pair(const float* st, const float2* tw, int Hv, int grp, int k, float (&re)[FQ_PER],
                                                   float (&im)[FQ_PER], float (&re2)[FQ_PER], float (&im2)[FQ_PER]) {
    const f32x4* s4 = reinterpret_cast<const f32x4*>(st) + 2 * grp;
    float A[FQ_PER] = {0.f, 0.f, 0.f, 0.f}, B[FQ_PER] = {0.f, 0.f, 0.f, 0.f}, C[FQ_PER] = {0.f, 0.f, 0.f, 0.f},
          E[FQ_PER] = {0.f, 0.f, 0.f, 0.f};
    int idx = 0;
#pragma unroll 4
    for (int t = 0; t < Hv; ++t) {
        const float2 cs = tw[idx];
        const f32x4 p = s4[t * (FQ_CROW / 4)], q = s4[t * (FQ_CROW / 4) + 1];
        const float vr[FQ_PER] = {p[0], p[2], q[0], q[2]}, vi[FQ_PER] = {p[1], p[3], q[1], q[3]};
#pragma unroll
        for (int j = 0; j < FQ_PER; ++j) {
            A[j] = fmaf(vr[j], cs.x, A[j]);
            B[j] = fmaf(vi[j], cs.y, B[j]);
            C[j] = fmaf(vi[j], cs.x, C[j]);
            E[j] = fmaf(vr[j], cs.y, E[j]);
        }
        idx += k;
        if (idx >= Hv) idx -= Hv;
    }
#pragma unroll
    for (int j = 0; j < FQ_PER; ++j) {
        const float rp = A[j] + B[j], rm = A[j] - B[j], ip = C[j] + E[j], im_ = C[j] - E[j];
        re[j] = SIGN < 0 ? rp : rm;
        im[j] = SIGN < 0 ? im_ : ip;
        re2[j] = SIGN < 0 ? rm : rp;
        im2[j] = SIGN < 0 ? ip : im_;
    }
}

__device__ __forceinline__ float fq_hermitian_weight(int kw, int Wv) { return (kw == 0 || 2 * kw == Wv) ? 1.f : 2.f; }

// ---- forward 1: workgroup = (image, plane, block of 8 view rows) -> work [N][C'][Hv][Wh][2] ------------------------------------
__global__ void __launch_bounds__(SISR_BLOCK) freq_rows_fwd_kernel(const float* __restrict__ a, const float* __restrict__ b, FreqGeom g,
                                                                   float* __restrict__ work) {
    __shared__ float2 tw[SISR_FREQ_MAX_SIDE];
    __shared__ __attribute__((aligned(16))) float sd[SISR_FREQ_MAX_SIDE * FQ_RPAD];      // [x][8 rows + 4]
    const int tid = threadIdx.x, nt = blockDim.x;
    const int per_image = g.planes * g.rblocks;
    const int n = blockIdx.x / per_image, r = blockIdx.x - n * per_image;
    const int plane = r / g.rblocks, y0 = (r - plane * g.rblocks) * FQ_LINES;
    const int64_t plane_elems = (int64_t)g.H * g.W;
    const int64_t base = ((int64_t)n * g.C + (g.luma ? 0 : plane)) * plane_elems;
    for (int i = tid; i < FQ_LINES * g.Wv; i += nt) {
        const int ly = i / g.Wv, x = i - ly * g.Wv;
        float v = 0.f;
        if (y0 + ly < g.Hv) {
            const int64_t off = base + (int64_t)(y0 + ly + g.crop) * g.W + (x + g.crop);
            v = fq_load(a, off, plane_elems, g.luma) - fq_load(b, off, plane_elems, g.luma);
        }
        sd[x * FQ_RPAD + ly] = v;
    }
    fq_twiddles(tw, g.Wv);
    float2* out = reinterpret_cast<float2*>(work) + ((int64_t)n * g.planes + plane) * g.Hv * g.Wh;
    for (int it = tid; it < FQ_GROUPS * g.Wh; it += nt) {
        const int grp = it / g.Wh, kw = it - grp * g.Wh;
        const f32x4* s4 = reinterpret_cast<const f32x4*>(sd) + grp;
        float re[FQ_PER] = {0.f, 0.f, 0.f, 0.f}, im[FQ_PER] = {0.f, 0.f, 0.f, 0.f};
        int idx = 0;
#pragma unroll 4
        for (int x = 0; x < g.Wv; ++x) {
            const float2 cs = tw[idx];
            const f32x4 d = s4[x * (FQ_RPAD / 4)];
#pragma unroll
            for (int j = 0; j < FQ_PER; ++j) {
                re[j] = fmaf(d[j], cs.x, re[j]);
                im[j] = fmaf(-d[j], cs.y, im[j]);
            }
            idx += kw;
            if (idx >= g.Wv) idx -= g.Wv;
        }
#pragma unroll
        for (int j = 0; j < FQ_PER; ++j) {
            const int y = y0 + grp * FQ_PER + j;
            if (y < g.Hv) out[(int64_t)y * g.Wh + kw] = make_float2(re[j], im[j]);
        }
    }
}

// the 8 columns kw0 .. of one (image, plane) of a [Hv][Wh] complex plane -> st [Hv][8][2]; F(value, kw) transforms on load
template <typename F>
__device__ __forceinline__ void fq_stage_columns(const float2* __restrict__ src, const FreqGeom& g, int kw0, float* st, F f) {
    for (int i = threadIdx.x, nt = blockDim.x; i < g.Hv * FQ_LINES; i += nt) {
        const int t = i / FQ_LINES, c = i - t * FQ_LINES, kw = kw0 + c;
        float2 v = make_float2(0.f, 0.f);
        if (kw < g.Wh) v = f(src[(int64_t)t * g.Wh + kw], kw);
        reinterpret_cast<float2*>(st)[i] = v;
    }
}

// ---- forward 2: workgroup = (image, plane, block of 8 kw columns) -> spec [N][C'][Hv][Wh][2] (or NULL), part [workgroup][2] --------
template <int KIND>
__global__ void __launch_bounds__(SISR_BLOCK) freq_cols_fwd_kernel(const float* __restrict__ work, FreqGeom g, float eps2,
                                                                   float half_alpha, float* __restrict__ spec,
                                                                   float* __restrict__ part) {
    __shared__ float2 tw[SISR_FREQ_MAX_SIDE];
    __shared__ __attribute__((aligned(16))) float st[SISR_FREQ_MAX_SIDE * FQ_CROW];
    __shared__ float red[2][SISR_BLOCK / 64];
    const int tid = threadIdx.x, nt = blockDim.x;
    const int np = blockIdx.x / g.cblocks, kw0 = (blockIdx.x - np * g.cblocks) * FQ_LINES;
    const int64_t plane_off = (int64_t)np * g.Hv * g.Wh;
    fq_stage_columns(reinterpret_cast<const float2*>(work) + plane_off, g, kw0, st, [](float2 v, int) { return v; });
    fq_twiddles(tw, g.Hv);
    float sum = 0.f, mx = 0.f;
    // one bin: store D, add its term
    auto bin = [&](int kh, int kw, float re, float im) {
        if (spec) reinterpret_cast<float2*>(spec)[plane_off + (int64_t)kh * g.Wh + kw] = make_float2(re, im);
        if (KIND == SISR_FREQ_FOCAL) {
            const float m2 = fmaf(re, re, im * im);
            if (m2 > 0.f) sum += fq_hermitian_weight(kw, g.Wv) * m2 * powf(m2, half_alpha);
            mx = fmaxf(mx, m2);
        } else if (KIND == SISR_FREQ_L1) {
            sum += fabsf(re) + fabsf(im);
        } else {
            sum += sqrtf(fmaf(re, re, eps2)) + sqrtf(fmaf(im, im, eps2));
        }
    };
    const int pairs = g.Hv / 2 + 1;                                   // kh = 0 .. Hv / 2, each with its partner Hv - kh
    for (int it = tid; it < FQ_GROUPS * pairs; it += nt) {
        const int grp = it / pairs, kh = it - grp * pairs, kh2 = g.Hv - kh;
        float re[FQ_PER], im[FQ_PER], re2[FQ_PER], im2[FQ_PER];
        fq_column_dft_pair<-1>(st, tw, g.Hv, grp, kh, re, im, re2, im2);
        const bool two = kh != 0 && kh2 != kh;                        // kh = 0 and the Nyquist row are their own partners
#pragma unroll
        for (int j = 0; j < FQ_PER; ++j) {
            const int kw = kw0 + grp * FQ_PER + j;
            if (kw >= g.Wh) continue;
            bin(kh, kw, re[j], im[j]);
            if (two) bin(kh2, kw, re2[j], im2[j]);
        }
    }
    sum = wave_sum(sum);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    if ((tid & 63) == 0) { red[0][tid >> 6] = sum; red[1][tid >> 6] = mx; }
    __syncthreads();
    if (tid == 0) {
        float s = red[0][0], m = red[1][0];
        for (int w = 1; w < (nt >> 6); ++w) { s += red[0][w]; m = fmaxf(m, red[1][w]); }
        part[2 * (int64_t)blockIdx.x] = s;
        part[2 * (int64_t)blockIdx.x + 1] = m;
    }
}

// ---- forward 3: one workgroup per image; thread p folds plane p's partials in block order in double ----------------------------
__global__ void __launch_bounds__(64) freq_finish_kernel(const float* __restrict__ part, int planes, int cblocks, int focal,
                                                         double half_alpha, double denom, float* __restrict__ loss,
                                                         float* __restrict__ pmax) {
    __shared__ double term[3];
    const int p = threadIdx.x;
    if (p < planes) {
        const float* q = part + 2 * ((int64_t)blockIdx.x * planes + p) * cblocks;
        double s = 0.0;
        float m = 0.f;
        for (int c = 0; c < cblocks; ++c) { s += (double)q[2 * c]; m = fmaxf(m, q[2 * c + 1]); }
        if (focal) {
            pmax[(int64_t)blockIdx.x * planes + p] = m;
            s = m > 0.f ? s / pow((double)m, half_alpha) : 0.0;
        }
        term[p] = s;
    }
    __syncthreads();
    if (p == 0) {
        double s = term[0];
        for (int q = 1; q < planes; ++q) s += term[q];
        loss[blockIdx.x] = (float)(s / denom);
    }
}

// ---- backward 1: workgroup = (image, plane, block of 8 kw columns); spec -> work [N][C'][Hv][Wh][2] -------------------------------
// coef: 1 / (C' Hv Wh 2) (L1, Charbonnier), 2 / ((Hv Wv)^2 C') (focal)
template <int KIND>
__global__ void __launch_bounds__(SISR_BLOCK) freq_cols_bwd_kernel(const float* __restrict__ spec, const float* __restrict__ gup,
                                                                   const float* __restrict__ pmax, FreqGeom g, float eps2,
                                                                   float half_alpha, float coef, float* __restrict__ work) {
    __shared__ float2 tw[SISR_FREQ_MAX_SIDE];
    __shared__ __attribute__((aligned(16))) float st[SISR_FREQ_MAX_SIDE * FQ_CROW];
    const int tid = threadIdx.x, nt = blockDim.x;
    const int np = blockIdx.x / g.cblocks, kw0 = (blockIdx.x - np * g.cblocks) * FQ_LINES;
    const int64_t plane_off = (int64_t)np * g.Hv * g.Wh;
    const float gs = gup[np / g.planes] * coef;
    const float mxv = KIND == SISR_FREQ_FOCAL ? pmax[np] : 0.f;
    const int Wv = g.Wv;
    fq_stage_columns(reinterpret_cast<const float2*>(spec) + plane_off, g, kw0, st, [=](float2 v, int kw) {
        if (KIND == SISR_FREQ_FOCAL) {
            float w = 0.f;
            if (mxv > 0.f) w = fminf(powf(fmaf(v.x, v.x, v.y * v.y) / mxv, half_alpha), 1.f);
            const float k = gs * fq_hermitian_weight(kw, Wv) * w;
            return make_float2(k * v.x, k * v.y);
        }
        if (KIND == SISR_FREQ_L1)
            return make_float2(v.x > 0.f ? gs : v.x < 0.f ? -gs : 0.f, v.y > 0.f ? gs : v.y < 0.f ? -gs : 0.f);
        return make_float2(gs * (v.x / sqrtf(fmaf(v.x, v.x, eps2))), gs * (v.y / sqrtf(fmaf(v.y, v.y, eps2))));
    });
    fq_twiddles(tw, g.Hv);
    const int pairs = g.Hv / 2 + 1;                                   // y = 0 .. Hv / 2, each with its partner Hv - y
    for (int it = tid; it < FQ_GROUPS * pairs; it += nt) {
        const int grp = it / pairs, y = it - grp * pairs, y2 = g.Hv - y;
        float re[FQ_PER], im[FQ_PER], re2[FQ_PER], im2[FQ_PER];
        fq_column_dft_pair<1>(st, tw, g.Hv, grp, y, re, im, re2, im2);
        const bool two = y != 0 && y2 != y;
#pragma unroll
        for (int j = 0; j < FQ_PER; ++j) {
            const int kw = kw0 + grp * FQ_PER + j;
            if (kw >= g.Wh) continue;
            reinterpret_cast<float2*>(work)[plane_off + (int64_t)y * g.Wh + kw] = make_float2(re[j], im[j]);
            if (two) reinterpret_cast<float2*>(work)[plane_off + (int64_t)y2 * g.Wh + kw] = make_float2(re2[j], im2[j]);
        }
    }
}

// ---- backward 2: workgroup = (image, plane, block of 8 rows of the WHOLE image); work -> da / db ---------------------------------
template <bool WA, bool WB>
__global__ void __launch_bounds__(SISR_BLOCK) freq_rows_bwd_kernel(const float* __restrict__ work, FreqGeom g, float* __restrict__ da,
                                                                   float* __restrict__ db) {
    __shared__ float2 tw[SISR_FREQ_MAX_SIDE];
    __shared__ __attribute__((aligned(16))) float su[FQ_MAX_WH * FQ_CPAD];                // [kw][8 rows][2] + 4
    const int tid = threadIdx.x, nt = blockDim.x;
    const int per_image = g.planes * g.iblocks;
    const int n = blockIdx.x / per_image, r = blockIdx.x - n * per_image;
    const int plane = r / g.iblocks, y0 = (r - plane * g.iblocks) * FQ_LINES;           // y0: a row of the whole image
    const float2* src = reinterpret_cast<const float2*>(work) + ((int64_t)n * g.planes + plane) * g.Hv * g.Wh;
    for (int i = tid; i < FQ_LINES * g.Wh; i += nt) {
        const int ly = i / g.Wh, kw = i - ly * g.Wh;
        const int yv = y0 + ly - g.crop;
        float2 v = make_float2(0.f, 0.f);
        if (yv >= 0 && yv < g.Hv) v = src[(int64_t)yv * g.Wh + kw];
        *reinterpret_cast<float2*>(su + kw * FQ_CPAD + 2 * ly) = v;
    }
    fq_twiddles(tw, g.Wv);
    const int64_t plane_elems = (int64_t)g.H * g.W;
    const int64_t base = ((int64_t)n * g.C + (g.luma ? 0 : plane)) * plane_elems;
    // one pixel (row y, column x of the whole image) of the plane's gradient v: the view's transpose
    auto put = [&](int y, int x, float v) {
        const int64_t off = base + (int64_t)y * g.W + x;
        if (g.luma) {
            const float v0 = 0.299f * v, v1 = 0.587f * v, v2 = 0.114f * v;
            if (WA) { da[off] = v0; da[off + plane_elems] = v1; da[off + 2 * plane_elems] = v2; }
            if (WB) { db[off] = -v0; db[off + plane_elems] = -v1; db[off + 2 * plane_elems] = -v2; }
        } else {
            if (WA) da[off] = v;
            if (WB) db[off] = -v;
        }
    };
    // the view's columns in pairs (xv, Wv - xv): conjugate twiddles, so A = sum ur cos and B = sum ui sin give A - B and A + B.
    // Rows outside the view were staged as zeros: their sums are exact zeros
    const int pairs = g.Wv / 2 + 1;
    for (int it = tid; it < FQ_GROUPS * pairs; it += nt) {
        const int grp = it / pairs, xv = it - grp * pairs, xv2 = g.Wv - xv;
        const f32x4* s4 = reinterpret_cast<const f32x4*>(su) + 2 * grp;
        float A[FQ_PER] = {0.f, 0.f, 0.f, 0.f}, B[FQ_PER] = {0.f, 0.f, 0.f, 0.f};
        int idx = 0;
#pragma unroll 4
        for (int kw = 0; kw < g.Wh; ++kw) {
            const float2 cs = tw[idx];
            const f32x4 p = s4[kw * (FQ_CPAD / 4)], q = s4[kw * (FQ_CPAD / 4) + 1];
            A[0] = fmaf(p[0], cs.x, A[0]); B[0] = fmaf(p[1], cs.y, B[0]);
            A[1] = fmaf(p[2], cs.x, A[1]); B[1] = fmaf(p[3], cs.y, B[1]);
            A[2] = fmaf(q[0], cs.x, A[2]); B[2] = fmaf(q[1], cs.y, B[2]);
            A[3] = fmaf(q[2], cs.x, A[3]); B[3] = fmaf(q[3], cs.y, B[3]);
            idx += xv;
            if (idx >= g.Wv) idx -= g.Wv;
        }
        const bool two = xv != 0 && xv2 != xv;
#pragma unroll
        for (int j = 0; j < FQ_PER; ++j) {
            const int y = y0 + grp * FQ_PER + j;
            if (y >= g.H) continue;
            put(y, xv + g.crop, A[j] - B[j]);
            if (two) put(y, xv2 + g.crop, A[j] + B[j]);
        }
    }
    // the cropped columns of these rows: exact zeros (the cropped rows came out as zeros above)
    const int bw = g.W - g.Wv;
    for (int it = tid; it < FQ_LINES * bw; it += nt) {
        const int ly = it / bw, bx = it - ly * bw;
        if (y0 + ly < g.H) put(y0 + ly, bx < g.crop ? bx : bx + g.Wv, 0.f);
    }
}

// threads for `outputs` output indices (or pairs) per line: 2 groups of 4 lines each, whole waves, at most SISR_BLOCK
static unsigned freq_block(int outputs) {
    const int items = FQ_GROUPS * outputs;
    return (unsigned)(items >= SISR_BLOCK ? SISR_BLOCK : (items + 63) / 64 * 64);
}

static bool freq_scalars_ok(int kind, float eps, float alpha) {
    return kind >= SISR_FREQ_L1 && kind <= SISR_FREQ_FOCAL && eps >= 0.f && alpha > 0.f && alpha <= 4.f;      // (a NaN fails)
}

extern "C" int sisr_freq_loss_ws_floats(int32_t N, int32_t C, int32_t H, int32_t W, int32_t crop, int32_t luma, int32_t which) {
    FreqGeom g;
    const int e = freq_geom(N, C, H, W, crop, luma, g);
    if (e) return e;
    int64_t floats;
    if (which == 0) floats = freq_spec_floats(N, g) + 2 * (int64_t)N * g.planes * g.cblocks;
    else if (which == 1 || which == 3) floats = freq_spec_floats(N, g);
    else if (which == 2) floats = (int64_t)N * g.planes;
    else return SISR_E_BADARG;
    return floats > INT32_MAX ? SISR_E_TOOBIG : (int)floats;
}

extern "C" int sisr_freq_loss_fwd(const float* a, const float* b, int32_t N, int32_t C, int32_t H, int32_t W, int32_t crop,
                                  int32_t luma, int32_t kind, float eps, float alpha, float* work, float* spec, float* pmax,
                                  float* loss, void* stream) {
    const int ws = sisr_freq_loss_ws_floats(N, C, H, W, crop, luma, 0);
    if (ws < 0) return ws;
    if (!a || !b || !work || !loss || !freq_scalars_ok(kind, eps, alpha) || (kind == SISR_FREQ_FOCAL && !pmax)) return SISR_E_BADARG;
    FreqGeom g;
    freq_geom(N, C, H, W, crop, luma, g);
    const int64_t row_wgs = (int64_t)N * g.planes * g.rblocks, col_wgs = (int64_t)N * g.planes * g.cblocks;
    float* part = work + freq_spec_floats(N, g);
    hipStream_t st = sisr_stream(stream);
    hipLaunchKernelGGL(freq_rows_fwd_kernel, dim3((unsigned)row_wgs), dim3(freq_block(g.Wh)), 0, st, a, b, g, work);
    SISR_CHECK_LAUNCH();
    const float half_alpha = 0.5f * alpha;
#define FQ_COLS_FWD(KIND)                                                                                                    \
    hipLaunchKernelGGL((freq_cols_fwd_kernel<KIND>), dim3((unsigned)col_wgs), dim3(freq_block(g.Hv / 2 + 1)), 0, st, (const float*)work, g, \
                       eps * eps, half_alpha, spec, part)
    if (kind == SISR_FREQ_L1) FQ_COLS_FWD(SISR_FREQ_L1);
    else if (kind == SISR_FREQ_CHARBONNIER) FQ_COLS_FWD(SISR_FREQ_CHARBONNIER);
    else FQ_COLS_FWD(SISR_FREQ_FOCAL);
#undef FQ_COLS_FWD
    SISR_CHECK_LAUNCH();
    const double hw = (double)g.Hv * g.Wv;
    const double denom = kind == SISR_FREQ_FOCAL ? hw * hw * g.planes : 2.0 * g.planes * g.Hv * g.Wh;
    hipLaunchKernelGGL(freq_finish_kernel, dim3((unsigned)N), dim3(64), 0, st, (const float*)part, g.planes, g.cblocks,
                       kind == SISR_FREQ_FOCAL ? 1 : 0, (double)half_alpha, denom, loss, pmax);
    SISR_CHECK_LAUNCH();
    return 0;
}

extern "C" int sisr_freq_loss_bwd(const float* spec, const float* pmax, const float* gup, int32_t N, int32_t C, int32_t H, int32_t W,
                                  int32_t crop, int32_t luma, int32_t kind, float eps, float alpha, float* work, float* da, float* db,
                                  void* stream) {
    const int ws = sisr_freq_loss_ws_floats(N, C, H, W, crop, luma, 3);
    if (ws < 0) return ws;
    if (!spec || !gup || !work || (!da && !db) || !freq_scalars_ok(kind, eps, alpha) || (kind == SISR_FREQ_FOCAL && !pmax))
        return SISR_E_BADARG;
    FreqGeom g;
    freq_geom(N, C, H, W, crop, luma, g);
    const int64_t col_wgs = (int64_t)N * g.planes * g.cblocks, img_wgs = (int64_t)N * g.planes * g.iblocks;
    if (img_wgs > INT32_MAX) return SISR_E_TOOBIG;
    const double hw = (double)g.Hv * g.Wv;
    const float coef = (float)(kind == SISR_FREQ_FOCAL ? 2.0 / (hw * hw * g.planes) : 1.0 / (2.0 * g.planes * g.Hv * g.Wh));
    hipStream_t st = sisr_stream(stream);
#define FQ_COLS_BWD(KIND)                                                                                                       \
    hipLaunchKernelGGL((freq_cols_bwd_kernel<KIND>), dim3((unsigned)col_wgs), dim3(freq_block(g.Hv / 2 + 1)), 0, st, spec, gup, pmax, g, eps * eps, \
                       0.5f * alpha, coef, work)
    if (kind == SISR_FREQ_L1) FQ_COLS_BWD(SISR_FREQ_L1);
    else if (kind == SISR_FREQ_CHARBONNIER) FQ_COLS_BWD(SISR_FREQ_CHARBONNIER);
    else FQ_COLS_BWD(SISR_FREQ_FOCAL);
#undef FQ_COLS_BWD
    SISR_CHECK_LAUNCH();
#define FQ_ROWS_BWD(WA, WB)                                                                                                  \
    hipLaunchKernelGGL((freq_rows_bwd_kernel<WA, WB>), dim3((unsigned)img_wgs), dim3(freq_block(g.Wv / 2 + 1)), 0, st, (const float*)work, g, da, db)
    if (da && db) FQ_ROWS_BWD(true, true);
    else if (da) FQ_ROWS_BWD(true, false);
    else FQ_ROWS_BWD(false, true);
#undef FQ_ROWS_BWD
    SISR_CHECK_LAUNCH();
    return 0;
}
