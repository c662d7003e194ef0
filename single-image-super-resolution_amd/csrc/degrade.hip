// degrade.hip -- the classical super-resolution degradation LR = clamp((HR (*) k) resampled + sigma_n z) on the device, forward and
// backward: a per-sample blur kernel, the bicubic resampling of utils.lr_from_hr (the taps of sisr_cubic.h),
// per-sample Gaussian noise, the clamp to [-1, 1].
//   degrade_draw_kernel  one workgroup, one wave per sample: step count t (device memory) -> kernels [B][K][K], noise_sigma [B], drawn_step = t; t -> t + 1;
//   degrade_fwd_kernel   one workgroup per LR tile and (n, c): HR footprint -> LDS (the kernel's weights: scalar loads), blur of the pixels the
//                        tile's taps read -> LDS, bicubic, noise, clamp, one coalesced store of y.  No intermediate touches HBM;
//   degrade_bwd_kernel   one workgroup per HR tile and (n, c): R^T (dy * mask) over the tile plus halo -> LDS, B^T (the flipped
//                        kernel) over the tile's PADDED coordinates -> LDS, then the fold of the replicate border onto its pixels.
//                        Gather form, fixed order, no atomics: the same bits on every call.
// Random numbers: the draws and tags of sisr_philox.h, one text for host and device (sisr_degrade_params_host / _noise_host are the
// same arithmetic without a GPU).  Plain vector stores only.  A drawn kernel's weights, sum and store are one code for both draws.
// The second-order model at the end of the file: degrade_draw_mix_kernel (family, noise row and final sinc
// filter of a sample) and degrade_noise_fwd_kernel / _bwd_kernel (Gaussian or shot noise, colour or grey, the clamp), elementwise.
#include "sisr_dev.h"
#include "sisr_cubic.h"
#include "sisr_philox.h"

#include <algorithm>
#include <cmath>

#define DG_KMAX 21
#define DG_PI 3.14159265358979323846f

// ---- random numbers --------------------------------------------------------------------------------------------------------------
struct DegradeDrawArgs {
    uint64_t seed;
    int rank, B, K, aniso;
    float lo, hi, nlo, nhi;
};

// parameters of sample b at step t: p = { sigma1, sigma2, theta, sigma_n }
__host__ __device__ __forceinline__ void degrade_draw_params(const DegradeDrawArgs& a, int64_t t, int b, float p[4]) {
    uint32_t r[4];
    draw_words(a.seed, t, (uint32_t)b, DRAW_TAG_PARAMS | (uint32_t)a.rank, r);
    p[0] = a.lo + (a.hi - a.lo) * draw_uniform(r[0]);
    p[1] = a.aniso ? a.lo + (a.hi - a.lo) * draw_uniform(r[1]) : p[0];
    p[2] = DG_PI * draw_uniform(r[2]);
    p[3] = a.nlo + (a.nhi - a.nlo) * draw_uniform(r[3]);
}

// z of output element e: group g = e / 4 draws four words, Box-Muller on (u0, u1) and (u2, u3), element e takes z[e mod 4]
__host__ __device__ __forceinline__ float degrade_noise_z_tagged(uint64_t seed, int64_t t, uint32_t tag_rank, int64_t e) {
    uint32_t r[4];
    draw_words(seed, t, (uint32_t)(e >> 2), tag_rank, r);
    const int j = (int)(e & 3);
    const float rad = sqrtf(-2.0f * draw_log_uniform(r[j & 2]));
    const float ang = 2.0f * DG_PI * draw_uniform(r[(j & 2) + 1]);
    return rad * ((j & 1) ? sinf(ang) : cosf(ang));
}
__host__ __device__ __forceinline__ float degrade_noise_z(uint64_t seed, int64_t t, int rank, int64_t e) {
    return degrade_noise_z_tagged(seed, t, DRAW_TAG_NOISE | (uint32_t)rank, e);
}

static bool degrade_draw_args_ok(const DegradeDrawArgs& a) {
    if (a.B < 1 || a.K < 1 || a.K > DG_KMAX || !(a.K & 1)) return false;
    if (a.rank < 0 || a.rank >= DRAW_RANK_LIMIT) return false;
    if (!(a.lo > 0.f) || !(a.lo <= a.hi) || !(a.hi < INFINITY)) return false;
    return a.nlo >= 0.f && a.nlo <= a.nhi && a.nhi < INFINITY;
}

// ---- one drawn kernel: its weights, their sum, the normalised store (both draws; the seven families are section 25's) -----------------
#define DG_FAMILY_SINC 6                          // 0 .. 5 index kernel_probs: iso, aniso, generalized_iso / _aniso, plateau_iso / _aniso
struct MixKernel {                                 // params row = family, k_eff, sigma1, sigma2, theta, beta, omega, on
    int family, k_eff, on;
    float s1, s2, theta, beta, omega;
};

// the first-order draw p = { sigma1, sigma2, theta, .. }: the anisotropic Gaussian at full size, rotated even where the sigmas are equal
__host__ __device__ __forceinline__ MixKernel degrade_gaussian(int K, const float p[4]) { return {1, K, 1, p[0], p[1], p[2], 0.f, 0.f}; }

// Bessel J1 for x >= 0 in double (arguments reach pi sqrt(2) 10 = 44.4): below 12 the power series sum_k (-1)^k (x/2)^(2k+1) /
// (k! (k+1)!) (largest term 4.2e3: 5e-13 of cancellation), from 12 on Hankel's expansion sqrt(2 / (pi x)) (P cos c - Q sin c),
// c = x - 3 pi / 4, with a_k = a_(k-1) (4 - (2k - 1)^2) / (8 k): P = sum (-1)^j a_2j / x^2j, Q = sum (-1)^j a_(2j+1) / x^(2j+1),
// twelve terms.  Within 1e-11 of the integral definition on [0, 47].
__host__ __device__ __forceinline__ double dg_j1(double x) {
    if (x < 12.0) {
        const double h = 0.5 * x, h2 = h * h;
        double term = h, sum = h;
#pragma unroll
        for (int k = 1; k <= 32; ++k) {
            term *= h2 * (-1.0 / (double)(k * (k + 1)));          // (a constant per unrolled step: no division at run time)
            sum += term;
        }
        return sum;
    }
    const double inv = 1.0 / x;
    double t = 1.0, P = 1.0, Q = 0.0;
#pragma unroll
    for (int k = 1; k <= 12; ++k) {
        t *= ((4.0 - (double)((2 * k - 1) * (2 * k - 1))) / (8.0 * (double)k)) * inv;
        const double s = ((k >> 1) & 1) ? -t : t;
        if (k & 1) Q += s;
        else P += s;
    }
    const double c = x - 2.35619449019234492885;
    return sqrt(0.63661977236758134308 / x) * (P * cos(c) - Q * sin(c));
}

// unnormalised weight of tap i = (dy + R) K + (dx + R); cs, sn = cosf, sinf of theta
__host__ __device__ __forceinline__ float mix_weight(int i, int K, const MixKernel& k, float cs, float sn) {
    const int R = (K - 1) / 2, Re = (k.k_eff - 1) / 2;
    const int iy = i / K - R, ix = i % K - R;
    if (!k.on) return iy == 0 && ix == 0 ? 1.f : 0.f;
    if (iy < -Re || iy > Re || ix < -Re || ix > Re) return 0.f;
    if (k.family == DG_FAMILY_SINC) {
        const double w = (double)k.omega;
        if (iy == 0 && ix == 0) return (float)(w * w / (4.0 * 3.14159265358979323846));
        const double r = sqrt((double)(ix * ix + iy * iy));
        return (float)(w * dg_j1(w * r) / (2.0 * 3.14159265358979323846 * r));
    }
    const float dy = (float)iy, dx = (float)ix;
    const float u = cs * dx + sn * dy, v = -sn * dx + cs * dy;
    const float q = u * u / (k.s1 * k.s1) + v * v / (k.s2 * k.s2);
    if (k.family < 2) return expf(-0.5f * q);
    const float qb = powf(q, k.beta);
    return k.family < 4 ? expf(-0.5f * qb) : 1.f / (qb + 1.f);
}

// The K^2 <= 448 weights of a sample sit 7 to a lane, tap i = lane + 64 m.  Their sum in a FIXED order: each lane adds its own,
// m ascending; the 64 partial sums are added pairwise, l and l + o for o = 32, 16 .. 1 (wave_sum's butterfly).  The host adds
// in the same order.
#define DG_PER_LANE ((DG_KMAX * DG_KMAX + 63) / 64)
static float degrade_sum_host(const float* w, int KK) {
    float part[64];
    for (int l = 0; l < 64; ++l) {
        part[l] = 0.f;
        for (int m = 0; m < DG_PER_LANE; ++m) part[l] += l + 64 * m < KK ? w[l + 64 * m] : 0.f;
    }
    for (int o = 32; o > 0; o >>= 1)
        for (int l = 0; l < o; ++l) part[l] += part[l + o];
    return part[0];
}

// one kernel of one sample by one wave: the weights 7 to a lane, their sum in degrade_sum_host's order, the normalised store
__device__ __forceinline__ void mix_store_kernel(const MixKernel& k, int K, int lane, float* __restrict__ dst) {
    const int KK = K * K;
    const float cs = cosf(k.theta), sn = sinf(k.theta);
    float w[DG_PER_LANE], part = 0.f;
#pragma unroll
    for (int m = 0; m < DG_PER_LANE; ++m) {
        const int i = lane + 64 * m;
        w[m] = i < KK ? mix_weight(i, K, k, cs, sn) : 0.f;
        part += w[m];
    }
    const float sum = wave_sum(part);
#pragma unroll
    for (int m = 0; m < DG_PER_LANE; ++m)
        if (lane + 64 * m < KK) dst[lane + 64 * m] = w[m] / sum;
}

static void mix_kernel_host(const MixKernel& k, int K, float* dst) {
    const int KK = K * K;
    const float cs = cosf(k.theta), sn = sinf(k.theta);
    float wk[DG_KMAX * DG_KMAX];
    for (int i = 0; i < KK; ++i) wk[i] = mix_weight(i, K, k, cs, sn);
    const float sum = degrade_sum_host(wk, KK);
    for (int i = 0; i < KK; ++i) dst[i] = wk[i] / sum;
}

// One workgroup, the step protocol of sisr_philox.h.  One wave per sample (b = wave, wave + 4, ..): no LDS, no further barrier.
__global__ void __launch_bounds__(SISR_BLOCK) degrade_draw_kernel(int64_t* __restrict__ step, DegradeDrawArgs a,
                                                                   float* __restrict__ kernels, float* __restrict__ noise_sigma,
                                                                   int64_t* __restrict__ drawn_step) {
    const int64_t t = draw_step_read(step);
    draw_step_advance(step, t, drawn_step);
    const int KK = a.K * a.K, lane = threadIdx.x & 63;
    for (int b = threadIdx.x >> 6; b < a.B; b += SISR_BLOCK / 64) {
        float p[4];
        degrade_draw_params(a, t, b, p);
        mix_store_kernel(degrade_gaussian(a.K, p), a.K, lane, kernels + (int64_t)b * KK);
        if (lane == 0) noise_sigma[b] = p[3];
    }
}

// ---- blur ------------------------------------------------------------------------------------------------------------------------
// out[p][q] = sum_{i, j < K} k[i][j] src[(ry[p] + i) SP + rx[q] + j] for p < nry, q < nrx: the correlation of the LDS image `src`
// with the sample's kernel at the window origins the two lists name (`flip`: the kernel read back to front, the transpose).
// The weights never enter LDS: their address is the same in every lane, so they are read through the constant address space --
// scalar loads into SGPRs, a row of K at a time -- and the LDS serves the image alone.  K is a template argument so that a row
// unrolls.  Fixed order per output: i outer, j inner, fused multiply-add -- the same in both variants below.
typedef const float __attribute__((address_space(4))) * dg_const_ptr;

// row pitch (floats, a multiple of 4) of an image whose windows start at columns < span: the adjacent-column variant reads
// 4 ceil((K + 3) / 4) floats from column 4 g on, g < ceil(span / 4); never less than the span + K - 1 columns the windows cover
__host__ __device__ __forceinline__ int dg_pitch(int span, int K) { return 4 * ((span + 3) / 4 - 1) + 4 * ((K + 6) / 4); }

// column list dense (rx[q] == q): one item = row p and the FOUR ADJACENT columns 4 g .. 4 g + 3.  Per kernel row the item reads
// K + 3 consecutive floats once, as 16-byte LDS reads at 16-byte-aligned addresses (consecutive lanes on consecutive 16-byte slots:
// conflict-free), for its 4 K products: 0.29 LDS dwords per multiply-add at K = 21.  src and SP must be 16-byte aligned / a
// multiple of 4; columns >= nrx of the last item read what lies behind the footprint inside the pitch and are not stored.
template <int K>
__device__ __forceinline__ void dg_blur_adjacent(const float* __restrict__ src, int SP, const float* kg, bool flip,
                                                 const int* __restrict__ ry, int nry, int nrx, float* __restrict__ out, int OP) {
    constexpr int NV = (K + 6) / 4;
    const dg_const_ptr kc = (dg_const_ptr)(uintptr_t)kg;
    const int G = (nrx + 3) >> 2;
    for (int it = threadIdx.x; it < nry * G; it += SISR_BLOCK) {
        const int p = it / G, g = it - p * G;
        const float* row = src + ry[p] * SP + 4 * g;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int i = 0; i < K; ++i, row += SP) {
            float w[K], xv[4 * NV];
#pragma unroll
            for (int j = 0; j < K; ++j) w[j] = flip ? kc[K * K - 1 - (i * K + j)] : kc[i * K + j];
#pragma unroll
            for (int m = 0; m < NV; ++m) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(row + 4 * m);
                xv[4 * m] = v[0]; xv[4 * m + 1] = v[1]; xv[4 * m + 2] = v[2]; xv[4 * m + 3] = v[3];
            }
#pragma unroll
            for (int j = 0; j < K; ++j) {
#pragma unroll
                for (int u = 0; u < 4; ++u) acc[u] = fmaf(w[j], xv[u + j], acc[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (4 * g + u < nrx) out[p * OP + 4 * g + u] = acc[u];
    }
}

// any column list: one item = row p and four columns q = g + j G (G = ceil(nrx / 4)), one 4-byte LDS read per product
template <int K>
__device__ __forceinline__ void dg_blur_listed(const float* __restrict__ src, int SP, const float* kg, bool flip,
                                               const int* __restrict__ ry, const int* __restrict__ rx, int nry, int nrx,
                                               float* __restrict__ out, int OP) {
    const dg_const_ptr kc = (dg_const_ptr)(uintptr_t)kg;
    const int G = (nrx + 3) >> 2;
    for (int it = threadIdx.x; it < nry * G; it += SISR_BLOCK) {
        const int p = it / G, g = it - p * G;
        int c[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) c[j] = rx[min(g + j * G, nrx - 1)];
        const float* row = src + ry[p] * SP;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int i = 0; i < K; ++i, row += SP) {
            float w[K];
#pragma unroll
            for (int j = 0; j < K; ++j) w[j] = flip ? kc[K * K - 1 - (i * K + j)] : kc[i * K + j];
#pragma unroll
            for (int j = 0; j < K; ++j) {
#pragma unroll
                for (int u = 0; u < 4; ++u) acc[u] = fmaf(w[j], row[c[u] + j], acc[u]);
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (g + j * G < nrx) out[p * OP + g + j * G] = acc[j];
    }
}

// rx == nullptr: the column list is dense
__device__ __forceinline__ void dg_blur(const float* __restrict__ src, int SP, const float* kg, int K, bool flip,
                                        const int* __restrict__ ry, const int* __restrict__ rx, int nry, int nrx,
                                        float* __restrict__ out, int OP) {
    switch (K) {
#define DG_BLUR_CASE(KT)                                                                       \
    case KT:                                                                                   \
        if (rx == nullptr) dg_blur_adjacent<KT>(src, SP, kg, flip, ry, nry, nrx, out, OP);     \
        else dg_blur_listed<KT>(src, SP, kg, flip, ry, rx, nry, nrx, out, OP);                 \
        break;
        DG_BLUR_CASE(1) DG_BLUR_CASE(3) DG_BLUR_CASE(5) DG_BLUR_CASE(7) DG_BLUR_CASE(9) DG_BLUR_CASE(11)
        DG_BLUR_CASE(13) DG_BLUR_CASE(15) DG_BLUR_CASE(17) DG_BLUR_CASE(19) DG_BLUR_CASE(21)
#undef DG_BLUR_CASE
    }
}

// ---- forward -----------------------------------------------------------------------------------------------------------------------
// One axis of a tile of T outputs from o0 on: the image indices its taps read lie in [lo, hi] (clamped).  The blurred pixels the
// tile needs are the outer product of a row list and a column list.  DENSE list: every index of [lo, hi]; SPARSE list: the 4 taps
// of each output, 4 T entries.  The host takes the shorter list per axis (degrade_axis_plan): dense below a ratio of about 4, where
// neighbouring outputs share taps, sparse above it, where blurring the whole footprint would blur pixels nobody reads.
struct DegradeAxis {
    int T, tiles, dense, n_cap, span_cap;      // list capacity, footprint capacity (indices of [lo, hi]) over all tiles
};

__host__ __device__ __forceinline__ int dg_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
// (cubic_setup's expressions: the first tap of the first output, the last tap of the last one)
__host__ __device__ __forceinline__ void dg_axis_range(int o0, int o1, float scale, int n_in, int& lo, int& hi) {
    lo = dg_clampi((int)floorf(scale * (float)o0) - 1, 0, n_in - 1);
    hi = dg_clampi((int)floorf(scale * (float)o1) + 2, 0, n_in - 1);
}

struct DegradeFwdArgs {
    const float *x, *k, *sigma;
    const int64_t* step;
    float* y;
    uint64_t seed;
    int rank, C, H, W, K, h, w, clampv;
    float sy, sx;
    DegradeAxis ay, ax;
};

// LDS: xs [(span_y + 2R)][XP] | bs [ny_cap][BP] | ry [ny_cap] | rx [nx_cap]
__global__ void __launch_bounds__(SISR_BLOCK) degrade_fwd_kernel(DegradeFwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float dg_lds[];
    const int K = a.K, R = (K - 1) >> 1;
    const int XP = dg_pitch(a.ax.span_cap, K), BP = a.ax.n_cap;
    float* xs = dg_lds;
    float* bs = xs + (a.ay.span_cap + 2 * R) * XP;
    int* ry = reinterpret_cast<int*>(bs + a.ay.n_cap * BP);
    int* rx = ry + a.ay.n_cap;
    const int nc = blockIdx.z, n = nc / a.C;
    const int oy0 = blockIdx.y * a.ay.T, ox0 = blockIdx.x * a.ax.T;
    const int oy1 = min(oy0 + a.ay.T, a.h) - 1, ox1 = min(ox0 + a.ax.T, a.w) - 1;
    int ylo, yhi, xlo, xhi;
    dg_axis_range(oy0, oy1, a.sy, a.H, ylo, yhi);
    dg_axis_range(ox0, ox1, a.sx, a.W, xlo, xhi);
    // (the host sized the capacities from these same expressions; the min() keeps a disagreement from ever leaving the buffers)
    const int spy = min(yhi - ylo + 1, a.ay.span_cap), spx = min(xhi - xlo + 1, a.ax.span_cap);
    const int nry = a.ay.dense ? spy : 4 * (oy1 - oy0 + 1), nrx = a.ax.dense ? spx : 4 * (ox1 - ox0 + 1);
    // the lists: offsets of the listed index from lo = the row (column) of xs where its K-tap window starts
    for (int i = threadIdx.x; i < nry; i += SISR_BLOCK) {
        int v = i;
        if (!a.ay.dense) {
            int idx[4]; float wt[4];
            cubic_setup(oy0 + (i >> 2), a.sy, a.H, idx, wt);
            v = min(max(idx[i & 3] - ylo, 0), spy - 1);
        }
        ry[i] = v;
    }
    for (int i = threadIdx.x; i < nrx; i += SISR_BLOCK) {
        int v = i;
        if (!a.ax.dense) {
            int idx[4]; float wt[4];
            cubic_setup(ox0 + (i >> 2), a.sx, a.W, idx, wt);
            v = min(max(idx[i & 3] - xlo, 0), spx - 1);
        }
        rx[i] = v;
    }
    // HR footprint with the replicate border applied: row r of xs is image row clamp(ylo - R + r)
    const float* img = a.x + (int64_t)nc * a.H * a.W;
    const int fh = spy + 2 * R, fw = spx + 2 * R;
    for (int i = threadIdx.x; i < fh * fw; i += SISR_BLOCK) {
        const int r = i / fw, c = i - r * fw;
        const int gy = min(max(ylo - R + r, 0), a.H - 1), gx = min(max(xlo - R + c, 0), a.W - 1);
        xs[r * XP + c] = img[(int64_t)gy * a.W + gx];
    }
    __syncthreads();
    dg_blur(xs, XP, a.k + (int64_t)n * K * K, K, false, ry, a.ax.dense ? nullptr : rx, nry, nrx, bs, BP);
    __syncthreads();
    // bicubic over the blurred pixels (the arithmetic of bicubic_fwd_kernel), noise, clamp
    const int tw = ox1 - ox0 + 1, th = oy1 - oy0 + 1;
    const bool noisy = a.sigma != nullptr;
    const float sg = noisy ? a.sigma[n] : 0.f;
    const int64_t t = noisy ? *a.step : 0;
    for (int i = threadIdx.x; i < th * tw; i += SISR_BLOCK) {
        const int ly = i / tw, lx = i - ly * tw;
        const int oy = oy0 + ly, ox = ox0 + lx;
        int iy[4], ix[4];
        float wy[4], wx[4];
        cubic_setup(oy, a.sy, a.H, iy, wy);
        cubic_setup(ox, a.sx, a.W, ix, wx);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            iy[q] = a.ay.dense ? min(max(iy[q] - ylo, 0), nry - 1) : 4 * ly + q;
            ix[q] = a.ax.dense ? min(max(ix[q] - xlo, 0), nrx - 1) : 4 * lx + q;
        }
        float acc = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float* row = bs + iy[q] * BP;
            const float r = row[ix[0]] * wx[0] + row[ix[1]] * wx[1] + row[ix[2]] * wx[2] + row[ix[3]] * wx[3];
            acc += r * wy[q];
        }
        const int64_t e = ((int64_t)nc * a.h + oy) * a.w + ox;
        if (noisy) acc += sg * degrade_noise_z(a.seed, t, a.rank, e);
        if (a.clampv) acc = fminf(fmaxf(acc, -1.f), 1.f);
        a.y[e] = acc;
    }
}

#define DG_LDS_BUDGET (64 * 1024)
#define DG_TILE_MAX 32

static DegradeAxis degrade_axis_plan(int T, int n_in, int n_out, float scale) {
    DegradeAxis p;
    p.T = T;
    p.tiles = (n_out + T - 1) / T;
    p.span_cap = 1;
    for (int i = 0; i < p.tiles; ++i) {
        int lo, hi;
        dg_axis_range(i * T, std::min(i * T + T, n_out) - 1, scale, n_in, lo, hi);
        p.span_cap = std::max(p.span_cap, hi - lo + 1);
    }
    p.dense = p.span_cap <= 4 * T;
    p.n_cap = p.dense ? p.span_cap : 4 * T;
    return p;
}

static int64_t degrade_fwd_lds(const DegradeAxis& ay, const DegradeAxis& ax, int K) {
    return 4 * ((int64_t)(ay.span_cap + K - 1) * dg_pitch(ax.span_cap, K) + (int64_t)ay.n_cap * ax.n_cap + ay.n_cap + ax.n_cap);
}

// the largest tile (at most 32 x 32 outputs, halving the axis with the larger footprint) whose LDS fits the budget.  A 1 x 1 tile
// reads 4 x 4 taps whatever the ratio, about (4 + 2R)^2 floats: every ratio can be staged, the extreme ones slowly.
static void degrade_fwd_plan(int H, int W, int K, int h, int w, float sy, float sx, DegradeAxis& ay, DegradeAxis& ax) {
    int TH = std::min(DG_TILE_MAX, h), TW = std::min(DG_TILE_MAX, w);
    for (;;) {
        ay = degrade_axis_plan(TH, H, h, sy);
        ax = degrade_axis_plan(TW, W, w, sx);
        if (degrade_fwd_lds(ay, ax, K) <= DG_LDS_BUDGET || (TH == 1 && TW == 1)) return;
        if (TW == 1 || (TH > 1 && ay.span_cap >= ax.span_cap)) TH = (TH + 1) / 2;
        else TW = (TW + 1) / 2;
    }
}

// ---- backward ----------------------------------------------------------------------------------------------------------------------
// dL/db at blurred pixel (iy, ix): the transpose of the interpolation in gather form (the sum of bicubic_bwd_kernel, same order)
__device__ __forceinline__ float dg_resample_bwd(const float* __restrict__ g, const float* __restrict__ v, int H, int W, int Ho, int Wo,
                                                 float sy, float sx, int iy, int ix) {
    int ylo, yhi, xlo, xhi;
    cubic_reach(iy, sy, Ho, ylo, yhi);
    cubic_reach(ix, sx, Wo, xlo, xhi);
    float acc = 0.f;
    for (int oy = ylo; oy <= yhi; ++oy) {
        const float wy = cubic_weight_of(oy, sy, H, iy);
        if (wy == 0.f) continue;
        float row = 0.f;
        for (int ox = xlo; ox <= xhi; ++ox) {
            const float wx = cubic_weight_of(ox, sx, W, ix);
            float gv = g[(int64_t)oy * Wo + ox];
            if (v != nullptr) {                    // clamp mask: gradient passes only strictly inside (-1, 1)
                const float c = v[(int64_t)oy * Wo + ox];
                if (!(c > -1.f && c < 1.f)) gv = 0.f;
            }
            row += wx * gv;
        }
        acc += wy * row;
    }
    return acc;
}

struct DegradeBwdArgs {
    const float *dy, *yc, *k;
    float* dx;
    int C, H, W, K, h, w;
    float sy, sx;
};

#define DG_BT 32                                   // HR pixels per tile side
#define DG_BP_MAX (DG_BT + DG_KMAX - 1)            // padded coordinates a tile can collect per axis: both borders fold R each
#define DG_BG_MAX (DG_BP_MAX + DG_KMAX - 1)        // ... and the gradient rows those read

// Tile [y0, y1] x [x0, x1] of the image.  A border pixel collects, besides its own, the R padded coordinates that the replicate
// border folds onto it: the tile's padded range is [py0, py1] with py0 = -R at the top border, py1 = H - 1 + R at the bottom one.
//   gs [gh][gw]  g = R^T (dy * mask) at blurred pixels [py0 - R, py1 + R] x ..., 0 outside the image;
//   ts [ph][pw]  t[p][q] = sum_{dy, dx} k[dy + R][dx + R] g[p - dy][q - dx]: dg_blur with the kernel flipped;
//   dx[y][x]     = sum of t over the padded coordinates that clamp to (y, x), rows ascending, columns ascending.
__global__ void __launch_bounds__(SISR_BLOCK) degrade_bwd_kernel(DegradeBwdArgs a) {
    __shared__ __attribute__((aligned(16))) float gs[DG_BG_MAX * DG_BG_MAX];      // pitch DG_BG_MAX = dg_pitch(52, 21)
    __shared__ float ts[DG_BP_MAX * DG_BP_MAX];
    __shared__ int lst[DG_BP_MAX];
    const int K = a.K, R = (K - 1) >> 1;
    const int nc = blockIdx.z, n = nc / a.C;
    const int y0 = blockIdx.y * DG_BT, x0 = blockIdx.x * DG_BT;
    const int y1 = min(y0 + DG_BT, a.H) - 1, x1 = min(x0 + DG_BT, a.W) - 1;
    const int py0 = y0 == 0 ? -R : y0, py1 = y1 == a.H - 1 ? a.H - 1 + R : y1;
    const int px0 = x0 == 0 ? -R : x0, px1 = x1 == a.W - 1 ? a.W - 1 + R : x1;
    const int ph = py1 - py0 + 1, pw = px1 - px0 + 1;          // <= DG_BP_MAX
    const int gh = ph + 2 * R, gw = pw + 2 * R;                // <= DG_BG_MAX
    for (int i = threadIdx.x; i < DG_BP_MAX; i += SISR_BLOCK) lst[i] = i;
    const float* g = a.dy + (int64_t)nc * a.h * a.w;
    const float* v = a.yc != nullptr ? a.yc + (int64_t)nc * a.h * a.w : nullptr;
    for (int i = threadIdx.x; i < gh * gw; i += SISR_BLOCK) {
        const int r = i / gw, c = i - r * gw;
        const int iy = py0 - R + r, ix = px0 - R + c;
        float val = 0.f;
        if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) val = dg_resample_bwd(g, v, a.H, a.W, a.h, a.w, a.sy, a.sx, iy, ix);
        gs[r * DG_BG_MAX + c] = val;
    }
    __syncthreads();
    // t[p][q] reads g rows p - R .. p + R = gs rows (p - py0) .. (p - py0) + 2R, with the kernel read back to front
    dg_blur(gs, DG_BG_MAX, a.k + (int64_t)n * K * K, K, true, lst, nullptr, ph, pw, ts, pw);
    __syncthreads();
    const int th = y1 - y0 + 1, tw = x1 - x0 + 1;
    float* out = a.dx + (int64_t)nc * a.H * a.W;
    for (int i = threadIdx.x; i < th * tw; i += SISR_BLOCK) {
        const int ly = i / tw, lx = i - ly * tw;
        const int y = y0 + ly, x = x0 + lx;
        const int fy0 = y == 0 ? -R : y, fy1 = y == a.H - 1 ? a.H - 1 + R : y;
        const int fx0 = x == 0 ? -R : x, fx1 = x == a.W - 1 ? a.W - 1 + R : x;
        float acc = 0.f;
        for (int p = fy0; p <= fy1; ++p) {
            float row = 0.f;
            for (int q = fx0; q <= fx1; ++q) row += ts[(p - py0) * pw + q - px0];
            acc += row;
        }
        out[(int64_t)y * a.W + x] = acc;
    }
}

// ---- entry points ------------------------------------------------------------------------------------------------------------------
static bool degrade_shape_ok(int N, int C, int H, int W, int K, int h, int w) {
    return N >= 1 && C >= 1 && C <= 4 && H >= 1 && W >= 1 && h >= 1 && w >= 1 && K >= 1 && K <= DG_KMAX && (K & 1);
}

extern "C" int sisr_degrade_draw(int64_t* step_dev, uint64_t seed, int32_t rank, int32_t B, int32_t K, float sigma_lo, float sigma_hi,
                                 int32_t anisotropic, float noise_lo, float noise_hi, float* kernels_dev, float* noise_sigma_dev,
                                 int64_t* drawn_step_dev, void* stream) {
    const DegradeDrawArgs a = {seed, rank, B, K, anisotropic != 0, sigma_lo, sigma_hi, noise_lo, noise_hi};
    if (!step_dev || !kernels_dev || !noise_sigma_dev || !drawn_step_dev || !degrade_draw_args_ok(a)) return SISR_E_BADARG;
    hipLaunchKernelGGL(degrade_draw_kernel, dim3(1), dim3(SISR_BLOCK), 0, sisr_stream(stream), step_dev, a, kernels_dev,
                       noise_sigma_dev, drawn_step_dev);
    SISR_CHECK_LAUNCH();
    return 0;
}

extern "C" int sisr_degrade_params_host(int64_t t, uint64_t seed, int32_t rank, int32_t B, int32_t K, float sigma_lo, float sigma_hi,
                                        int32_t anisotropic, float noise_lo, float noise_hi, float* kernels_host,
                                        float* noise_sigma_host, float* params_host) {
    const DegradeDrawArgs a = {seed, rank, B, K, anisotropic != 0, sigma_lo, sigma_hi, noise_lo, noise_hi};
    if (!kernels_host || !noise_sigma_host || t < 0 || !degrade_draw_args_ok(a)) return SISR_E_BADARG;
    for (int b = 0; b < B; ++b) {
        float p[4];
        degrade_draw_params(a, t, b, p);
        mix_kernel_host(degrade_gaussian(K, p), K, kernels_host + (int64_t)b * K * K);
        noise_sigma_host[b] = p[3];
        if (params_host)
            for (int i = 0; i < 4; ++i) params_host[4 * (int64_t)b + i] = p[i];
    }
    return 0;
}

extern "C" int sisr_degrade_noise_host(int64_t t, uint64_t seed, int32_t rank, int64_t first, int64_t count, float* z_host) {
    if (!z_host || t < 0 || rank < 0 || rank >= DRAW_RANK_LIMIT || first < 0 || count < 1) return SISR_E_BADARG;
    if (first + count > ((int64_t)1 << 34)) return SISR_E_TOOBIG;
    for (int64_t i = 0; i < count; ++i) z_host[i] = degrade_noise_z(seed, t, rank, first + i);
    return 0;
}

extern "C" int sisr_degrade_fwd(const float* x, const float* kernels, const float* noise_sigma, const int64_t* step_dev, uint64_t seed,
                                int32_t rank, float* y, int32_t N, int32_t C, int32_t H, int32_t W, int32_t K, int32_t h, int32_t w,
                                int32_t clampv, void* stream) {
    if (!x || !kernels || !y || (noise_sigma && !step_dev) || !degrade_shape_ok(N, C, H, W, K, h, w) || rank < 0 || rank >= DRAW_RANK_LIMIT)
        return SISR_E_BADARG;
    if ((int64_t)N * C * h * w >= ((int64_t)1 << 34)) return SISR_E_TOOBIG;
    if ((int64_t)N * C > 65535 || ((int64_t)h + DG_TILE_MAX - 1) / DG_TILE_MAX > 65535) return SISR_E_TOOBIG;      // grid.z, grid.y (before the plan walks the tiles)
    DegradeFwdArgs a = {x, kernels, noise_sigma, step_dev, y, seed, rank, C, H, W, K, h, w, clampv, ac_scale(H, h), ac_scale(W, w), {}, {}};
    degrade_fwd_plan(H, W, K, h, w, a.sy, a.sx, a.ay, a.ax);
    const int64_t lds = degrade_fwd_lds(a.ay, a.ax, K);
    if (lds > 160 * 1024) return SISR_E_UNSUPPORTED;       // (not reachable: a 1 x 1 tile needs (4 + 2R)^2 floats)
    if (a.ay.tiles > 65535) return SISR_E_TOOBIG;
    return sisr_launch<degrade_fwd_kernel>(dim3(a.ax.tiles, a.ay.tiles, N * C), dim3(SISR_BLOCK), (int)lds, SISR_LDS_BASE_DEFAULT,
                                           sisr_stream(stream), a);
}

extern "C" int sisr_degrade_bwd(const float* dy, const float* y_saved, const float* kernels, float* dx, int32_t N, int32_t C, int32_t H,
                                int32_t W, int32_t K, int32_t h, int32_t w, void* stream) {
    if (!dy || !kernels || !dx || !degrade_shape_ok(N, C, H, W, K, h, w)) return SISR_E_BADARG;
    const int ty = (H + DG_BT - 1) / DG_BT, tx = (W + DG_BT - 1) / DG_BT;
    if ((int64_t)N * C > 65535 || ty > 65535) return SISR_E_TOOBIG;
    const DegradeBwdArgs a = {dy, y_saved, kernels, dx, C, H, W, K, h, w, ac_scale(H, h), ac_scale(W, w)};
    hipLaunchKernelGGL(degrade_bwd_kernel, dim3(tx, ty, N * C), dim3(SISR_BLOCK), 0, sisr_stream(stream), a);
    SISR_CHECK_LAUNCH();
    return 0;
}

// ==== second-order degradation: the mixed kernel draw and the noise operator =================================
// Draws of sample b at step t: the four counters {t low, t high, b, DRAW_TAG_MIX_A .. _FINAL | rank} (which word decides what: the
// enum's comments, DESIGN.md section 25's table, mix_draw_sample), u_i = draw_uniform(r_i); an event of probability p happens when
// u <= p (u is in (0, 1]: p = 1 always, p = 0 never).  Everything is drawn whatever the earlier draws decided; a parameter the
// family does not use is stored as 0 (beta, omega), the iso forms and sinc store sigma2 = sigma1, theta = 0.
#define DG_MIX_BLOCK 512                          // the draw's one workgroup: 8 waves, 8 samples at a time (222 VGPRs: 1024 threads would spill)
#define DG_NOISE_NONE 0
#define DG_NOISE_GAUSSIAN 1
#define DG_NOISE_SHOT 2

struct MixDrawArgs {
    uint64_t seed;
    int rank, B;
    SisrDegradeMix m;
};

__host__ __device__ __forceinline__ void mix_philox(const MixDrawArgs& a, int64_t t, int b, uint32_t tag, float u[4]) {
    uint32_t r[4];
    draw_words(a.seed, t, (uint32_t)b, tag | (uint32_t)a.rank, r);
    for (int i = 0; i < 4; ++i) u[i] = draw_uniform(r[i]);
}

__host__ __device__ __forceinline__ int mix_k_eff(const SisrDegradeMix& m, float u) {
    const int cnt = (m.K - m.ksize_min) / 2 + 1, j = (int)((float)cnt * u);
    return m.ksize_min + 2 * (j < cnt - 1 ? j : cnt - 1);
}
__host__ __device__ __forceinline__ float mix_omega(int k_eff, float u) {
    const float lo = k_eff < 13 ? DG_PI / 3.f : DG_PI / 5.f;
    return lo + (DG_PI - lo) * u;
}

// the sample's kernel, its final filter and its noise row {mode, grey, amplitude, 0}
__host__ __device__ __forceinline__ void mix_draw_sample(const MixDrawArgs& a, int64_t t, int b, MixKernel& k, MixKernel& f, float noise[4]) {
    const SisrDegradeMix& m = a.m;
    float ua[4], ub[4], uc[4], uf[4];
    mix_philox(a, t, b, DRAW_TAG_MIX_A, ua);
    mix_philox(a, t, b, DRAW_TAG_MIX_B, ub);
    mix_philox(a, t, b, DRAW_TAG_MIX_C, uc);
    mix_philox(a, t, b, DRAW_TAG_MIX_FINAL, uf);
    k.on = ua[0] <= m.blur_prob;
    k.k_eff = mix_k_eff(m, ua[1]);
    k.family = ua[2] <= m.sinc_prob ? DG_FAMILY_SINC : draw_pick(m.kernel_probs, 6, ua[3]);
    const bool aniso = k.family == 1 || k.family == 3 || k.family == 5;
    k.s1 = m.sigma_lo + (m.sigma_hi - m.sigma_lo) * ub[0];
    k.s2 = aniso ? m.sigma_lo + (m.sigma_hi - m.sigma_lo) * ub[1] : k.s1;
    k.theta = aniso ? DG_PI * ub[2] : 0.f;
    k.beta = 0.f;
    if (k.family == 2 || k.family == 3) k.beta = m.beta_g_lo + (m.beta_g_hi - m.beta_g_lo) * ub[3];
    if (k.family == 4 || k.family == 5) k.beta = m.beta_p_lo + (m.beta_p_hi - m.beta_p_lo) * ub[3];
    k.omega = k.family == DG_FAMILY_SINC ? mix_omega(k.k_eff, uc[0]) : 0.f;
    const bool noisy = m.noise_hi > 0.f || m.shot_hi > 0.f;
    const bool gauss = uc[1] <= m.gaussian_prob;
    noise[0] = (float)(!noisy ? DG_NOISE_NONE : gauss ? DG_NOISE_GAUSSIAN : DG_NOISE_SHOT);
    noise[1] = noisy && uc[2] <= m.grey_prob ? 1.f : 0.f;
    noise[2] = !noisy ? 0.f : gauss ? m.noise_lo + (m.noise_hi - m.noise_lo) * uc[3] : m.shot_lo + (m.shot_hi - m.shot_lo) * uc[3];
    noise[3] = 0.f;
    f.on = uf[0] <= m.final_sinc_prob;
    f.family = DG_FAMILY_SINC;
    f.k_eff = mix_k_eff(m, uf[1]);
    f.omega = mix_omega(f.k_eff, uf[2]);
    f.s1 = f.s2 = 1.f;
    f.theta = f.beta = 0.f;
}

__host__ __device__ __forceinline__ void mix_params_row(const MixKernel& k, float p[8]) {
    p[0] = (float)k.family; p[1] = (float)k.k_eff; p[2] = k.s1; p[3] = k.s2;
    p[4] = k.theta; p[5] = k.beta; p[6] = k.omega; p[7] = (float)k.on;
}

static bool mix_prob_ok(float p) { return p >= 0.f && p <= 1.f; }
static bool mix_range_ok(float lo, float hi, bool positive) { return (positive ? lo > 0.f : lo >= 0.f) && lo <= hi && hi < INFINITY; }
static bool mix_args_ok(const MixDrawArgs& a) {
    const SisrDegradeMix& m = a.m;
    if (a.B < 1 || m.K < 1 || m.K > DG_KMAX || !(m.K & 1) || m.ksize_min < 1 || m.ksize_min > m.K || !(m.ksize_min & 1)) return false;
    if (a.rank < 0 || a.rank >= DRAW_RANK_LIMIT) return false;
    if (!mix_prob_ok(m.blur_prob) || !mix_prob_ok(m.sinc_prob) || !mix_prob_ok(m.gaussian_prob) || !mix_prob_ok(m.grey_prob) ||
        !mix_prob_ok(m.final_sinc_prob))
        return false;
    double sum = 0.0;
    for (int i = 0; i < 6; ++i) {
        if (!mix_prob_ok(m.kernel_probs[i])) return false;
        sum += (double)m.kernel_probs[i];
    }
    if (!(fabs(sum - 1.0) <= 1e-6)) return false;
    return mix_range_ok(m.sigma_lo, m.sigma_hi, true) && mix_range_ok(m.beta_g_lo, m.beta_g_hi, true) &&
           mix_range_ok(m.beta_p_lo, m.beta_p_hi, true) && mix_range_ok(m.noise_lo, m.noise_hi, false) &&
           mix_range_ok(m.shot_lo, m.shot_hi, false);
}

// degrade_draw_kernel's pattern: one workgroup, the step protocol, one wave per sample
__global__ void __launch_bounds__(DG_MIX_BLOCK) degrade_draw_mix_kernel(int64_t* __restrict__ step, MixDrawArgs a, float* __restrict__ kernels,
                                                                       float* __restrict__ final_kernels, float* __restrict__ params,
                                                                       float* __restrict__ noise_table, int64_t* __restrict__ drawn_step) {
    const int64_t t = draw_step_read(step);
    draw_step_advance(step, t, drawn_step);
    const int KK = a.m.K * a.m.K, lane = threadIdx.x & 63;
    for (int b = threadIdx.x >> 6; b < a.B; b += DG_MIX_BLOCK / 64) {
        MixKernel k, f;
        float noise[4], p[8];
        mix_draw_sample(a, t, b, k, f, noise);
        mix_store_kernel(k, a.m.K, lane, kernels + (int64_t)b * KK);
        if (final_kernels != nullptr) mix_store_kernel(f, a.m.K, lane, final_kernels + (int64_t)b * KK);
        mix_params_row(k, p);
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < 8; ++i) params[8 * (int64_t)b + i] = p[i];
#pragma unroll
            for (int i = 0; i < 4; ++i) noise_table[4 * (int64_t)b + i] = noise[i];
        }
    }
}

extern "C" int sisr_degrade_mix_bytes(void) { return (int)sizeof(SisrDegradeMix); }

extern "C" int sisr_degrade_draw_mix(int64_t* step_dev, uint64_t seed, int32_t rank, int32_t B, const SisrDegradeMix* mix, float* kernels_dev,
                                     float* final_kernels_dev, float* params_dev, float* noise_table_dev, int64_t* drawn_step_dev,
                                     void* stream) {
    if (!step_dev || !mix || !kernels_dev || !params_dev || !noise_table_dev || !drawn_step_dev) return SISR_E_BADARG;
    const MixDrawArgs a = {seed, rank, B, *mix};
    if (!mix_args_ok(a)) return SISR_E_BADARG;
    hipLaunchKernelGGL(degrade_draw_mix_kernel, dim3(1), dim3(DG_MIX_BLOCK), 0, sisr_stream(stream), step_dev, a, kernels_dev,
                       final_kernels_dev, params_dev, noise_table_dev, drawn_step_dev);
    SISR_CHECK_LAUNCH();
    return 0;
}

extern "C" int sisr_degrade_mix_host(int64_t t, uint64_t seed, int32_t rank, int32_t B, const SisrDegradeMix* mix, float* kernels_host,
                                     float* final_kernels_host, float* params_host, float* noise_table_host) {
    if (!mix || !kernels_host || !params_host || !noise_table_host || t < 0) return SISR_E_BADARG;
    const MixDrawArgs a = {seed, rank, B, *mix};
    if (!mix_args_ok(a)) return SISR_E_BADARG;
    const int KK = mix->K * mix->K;
    for (int b = 0; b < B; ++b) {
        MixKernel k, f;
        mix_draw_sample(a, t, b, k, f, noise_table_host + 4 * (int64_t)b);
        mix_kernel_host(k, mix->K, kernels_host + (int64_t)b * KK);
        if (final_kernels_host) mix_kernel_host(f, mix->K, final_kernels_host + (int64_t)b * KK);
        mix_params_row(k, params_host + 8 * (int64_t)b);
    }
    return 0;
}

extern "C" int sisr_degrade_noise_grey_host(int64_t t, uint64_t seed, int32_t rank, int64_t first, int64_t count, float* z_host) {
    if (!z_host || t < 0 || rank < 0 || rank >= DRAW_RANK_LIMIT || first < 0 || count < 1) return SISR_E_BADARG;
    if (first + count > ((int64_t)1 << 34)) return SISR_E_TOOBIG;
    for (int64_t i = 0; i < count; ++i) z_host[i] = degrade_noise_z_tagged(seed, t, DRAW_TAG_NOISE_GREY | (uint32_t)rank, first + i);
    return 0;
}

// ---- noise operator: y = clamp(x + n), n a constant under autograd ------------------------------------------------------------------
struct DegradeNoiseArgs {
    const float *x, *table;
    const int64_t* step;
    float* y;
    uint64_t seed;
    int rank, C, clampv;
    int64_t hw, pixels;                            // h w; N h w
};

// One thread per pixel (n, p), grid-stride: its C values, the sample's row {mode, grey, amplitude}.  Colour: z of element
// (n C + c) hw + p from the stream of sisr_degrade_fwd; grey: one z of pixel n hw + p under DRAW_TAG_NOISE_GREY, v = the luma.
__global__ void __launch_bounds__(SISR_BLOCK) degrade_noise_fwd_kernel(DegradeNoiseArgs a) {
    const int64_t t = *a.step;
    for (int64_t i = (int64_t)blockIdx.x * SISR_BLOCK + threadIdx.x; i < a.pixels; i += (int64_t)gridDim.x * SISR_BLOCK) {
        const int64_t n = i / a.hw, p = i - n * a.hw, base = n * a.C * a.hw + p;
        const int mode = (int)a.table[4 * n];
        const bool grey = a.table[4 * n + 1] != 0.f;
        const float amp = a.table[4 * n + 2];
        float v[4], nz[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = c < a.C ? a.x[base + c * a.hw] : 0.f;
        if (mode != DG_NOISE_NONE && grey) {
            const float l = a.C == 3 ? 0.299f * v[0] + 0.587f * v[1] + 0.114f * v[2] : (v[0] + v[1] + v[2] + v[3]) / (float)a.C;
            const float z = degrade_noise_z_tagged(a.seed, t, DRAW_TAG_NOISE_GREY | (uint32_t)a.rank, i);
            const float g = mode == DG_NOISE_GAUSSIAN ? amp * z : amp * 0.125f * sqrtf(fminf(fmaxf((l + 1.f) * 0.5f, 0.f), 1.f)) * z;
#pragma unroll
            for (int c = 0; c < 4; ++c) nz[c] = g;
        } else if (mode != DG_NOISE_NONE) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (c >= a.C) break;
                const float z = degrade_noise_z(a.seed, t, a.rank, base + c * a.hw);
                nz[c] = mode == DG_NOISE_GAUSSIAN ? amp * z : amp * 0.125f * sqrtf(fminf(fmaxf((v[c] + 1.f) * 0.5f, 0.f), 1.f)) * z;
            }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (c >= a.C) break;
            float r = v[c] + nz[c];
            if (a.clampv) r = fminf(fmaxf(r, -1.f), 1.f);
            a.y[base + c * a.hw] = r;
        }
    }
}

__global__ void __launch_bounds__(SISR_BLOCK) degrade_noise_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ ys,
                                                                        float* __restrict__ dx, int64_t count) {
    for (int64_t i = (int64_t)blockIdx.x * SISR_BLOCK + threadIdx.x; i < count; i += (int64_t)gridDim.x * SISR_BLOCK) {
        float g = dy[i];
        if (ys != nullptr) {                       // the product with the 0 / 1 mask, as written: a masked negative dy gives -0
            const float c = ys[i];
            g *= c > -1.f && c < 1.f ? 1.f : 0.f;
        }
        dx[i] = g;
    }
}

#define DG_NOISE_GRID_MAX 2048                     // 256 CUs x 8 workgroups; the grid-stride loop takes the rest
static int degrade_noise_grid(int64_t items) { return (int)std::min<int64_t>((items + SISR_BLOCK - 1) / SISR_BLOCK, DG_NOISE_GRID_MAX); }
static bool degrade_noise_shape_ok(int N, int C, int h, int w) { return N >= 1 && C >= 1 && C <= 4 && h >= 1 && w >= 1; }

extern "C" int sisr_degrade_noise_fwd(const float* x, const float* noise_table, const int64_t* step_dev, uint64_t seed, int32_t rank,
                                      float* y, int32_t N, int32_t C, int32_t h, int32_t w, int32_t clampv, void* stream) {
    if (!x || !noise_table || !step_dev || !y || !degrade_noise_shape_ok(N, C, h, w) || rank < 0 || rank >= DRAW_RANK_LIMIT) return SISR_E_BADARG;
    if ((int64_t)N * C * h * w >= ((int64_t)1 << 34)) return SISR_E_TOOBIG;
    const int64_t hw = (int64_t)h * w;
    const DegradeNoiseArgs a = {x, noise_table, step_dev, y, seed, rank, C, clampv, hw, (int64_t)N * hw};
    hipLaunchKernelGGL(degrade_noise_fwd_kernel, dim3(degrade_noise_grid(a.pixels)), dim3(SISR_BLOCK), 0, sisr_stream(stream), a);
    SISR_CHECK_LAUNCH();
    return 0;
}

extern "C" int sisr_degrade_noise_bwd(const float* dy, const float* y_saved, float* dx, int32_t N, int32_t C, int32_t h, int32_t w,
                                      void* stream) {
    if (!dy || !dx || !degrade_noise_shape_ok(N, C, h, w)) return SISR_E_BADARG;
    const int64_t count = (int64_t)N * C * h * w;
    if (count >= ((int64_t)1 << 34)) return SISR_E_TOOBIG;
    hipLaunchKernelGGL(degrade_noise_bwd_kernel, dim3(degrade_noise_grid(count)), dim3(SISR_BLOCK), 0, sisr_stream(stream), dy, y_saved,
                       dx, count);
    SISR_CHECK_LAUNCH();
    return 0;
}
