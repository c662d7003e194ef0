// toimage_bwd.hip -- the whole backward of the generator's LAST convolution (model_generator.py:52-53: 3x3, 64 -> 3, stride 1,
// pad 1, + Tanh) with fp32 tensors, in ONE pass over the step's two largest tensors: the upscale stage's pre-activation `pre`
// and the gradient `g` wrt its activated value (each [16,192,192,64] fp32 = 151 MB at the bench size).
//
// Separately this backward is three passes (profiles/r04_trace_step_order_fp32.txt): wgrad_toimage_f32_kernel reads act(pre)
// (77 us), the generic data gradient writes g (75 us), prelu_slope_partial_kernel reads g and pre again (48 + 6 us) -- 633 MB.
// The result needs pre read once and g written once: 316 MB.  One kernel on wgrad_toimage.hip's skeleton:
//   * 512 threads, one workgroup per CU, persistent over 8 x 32 pixel tiles (9 per CU at HR 192); `pre` is staged UNSHIFTED and
//     UNACTIVATED as [pixel][64] (64 KB), the 3-channel gradient halo dyt = dy * (1 - out^2) planar as [co][10 rows][40 columns];
//   * two such tile buffers: while tile t is contracted out of one, tile t + 1 -- requested a whole tile earlier -- is committed
//     to the other, and tile t + 2 is requested at once: one barrier per tile, loads always in flight;
//   * weight gradient, exactly wgrad_toimage_f32_kernel's contraction and order (its slabs are bit-identical):
//         D[ci 64][n = (ky', kx', co), 27 of 32] += lrelu(pre(q))[ci] * dyt(q + (ky' - 1, kx' - 1))[co]       K = pixels, 2 per MFMA
//     -- the PReLU is applied to the A operand as it is read, because the slope term needs pre itself (a slope of 0 loses it);
//   * data gradient on the same staged halo, exact v_mfma_f32_32x32x2_f32, K = 27 (co, ky, kx) in 15 steps:
//         G[pixel 32][ci 32] = sum_k dyt[co][pixel + (1 - ky, 1 - kx)] * W[co][ci][ky][kx]
//     the pixel operand is one 4-byte LDS read per step (lanes = consecutive pixels of a tile row), the weights live in 30
//     registers per lane for the whole launch (read once from the layer's packed FORWARD image).  The K order is the generic
//     kernel's for this layer (conv_fwd.hip on the plan CK = PS = 3, KROWP = 12: per tap row ky = 2, 1, 0 the nine (kx = 2, 1, 0;
//     co) products in pairs, the tenth slot zero), so g has the bits the separate data gradient gives and every gradient
//     upstream of it is unchanged -- 60 instead of 56 MFMAs per wave and tile (3 % of the matrix time);
//   * an accumulator register holds one pixel x one channel with lanes on consecutive channels: g is stored as 128-byte runs,
//     and the slope term  dslope += [pre <= 0] g * pre  reads pre from the staged tile (conflict-free: lanes = channels) -- pre
//     crosses HBM once;
//   * the eight waves split by ROLE: waves 0-3 run the weight gradient (64 MFMAs per tile, tile rows 2w, 2w + 1: the partition
//     and order of the 256-thread kernel), waves 4-7 the data gradient, slope term and store of the same rows (60 MFMAs); a SIMD
//     holds one wave of each role, and each fills the other's waits for its own LDS reads, conversions and stores (an fp32 MFMA
//     does not overlap its own wave's other instructions: with one wave per SIMD the kernel took 108 us, so 80).  The four
//     partial weight gradients meet in LDS at the end.  One slab per workgroup, every entry written (index walked with carries);
//   * the slope term is accumulated in DOUBLE (a product of two floats is exact there): per lane, then lanes and waves in a fixed
//     order, one double partial per workgroup; toimage_bwd_finish_kernel adds the partials in a fixed order and rounds ONCE to
//     fp32 -- the same bits from run to run, and a sum of 10^7 terms with heavy cancellation good to one fp32 rounding.
// Budget: LDS 2 x (65536 + 4800) + 64 bytes = 137 KB of 160; 243 VGPRs: 32 staged x values, 2 x 16 accumulators per role, 30
// weights, 15 halo offsets.  Floors at 16 x 192 x 192: 316 MB = 50 us at 6.3 TB/s; 62 MFMAs per 32 pixels = 34 us.
// Requirements (sisr_toimage_bwd_f32_eligible): the geometry above, H % 8 == 0, W % 32 == 0, fp32 tensors, tensor bytes < 2^31.
#include "sisr_dev.h"

#include <cstdlib>

#define TB_TH 8
#define TB_TW 32
#define TB_PS 64                           // floats per pre pixel in LDS
#define TB_XBYTES (TB_TH * TB_TW * TB_PS * 4)     // 65536
#define TB_GROWS (TB_TH + 2)               // gradient halo rows (origin = tile origin - 1)
#define TB_GW 40                           // gradient halo columns (origin = tile origin - 4: 16-byte aligned rows)
#define TB_GBYTES (3 * TB_GROWS * TB_GW * 4)      // 4800
#define TB_BUF (TB_XBYTES + TB_GBYTES)     // one tile buffer: 70336
#define TB_THREADS 512                     // eight waves: two per SIMD
#define TB_XITEMS 8                        // 16-byte pre items per thread and tile
#define TB_GITEMS 5                        // gradient halo elements per thread: 1200 = 4.7 x 256
#define TB_KSTEPS 15                       // data gradient: K = 3 tap rows x (9 products + a zero slot), 2 per MFMA

struct ToImageBwdArgs {
    const float *pre, *g1, *g2, *wpk;
    float *g, *slab, *bias_slab;
    double* dslope_part;
    const float* slope_p;
    float slope;
    int N, H, W;
    int tiles_x, per_img, total;
    int w_CK, w_PS, w_KROWP, w_CoutPad;
    int CK, PS, KROWP, CoutPad, slab_elems;
    long long slab_stride;
};

template <bool TANHB>
__global__ void __launch_bounds__(TB_THREADS, 1) toimage_bwd_f32_kernel(const ToImageBwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    // two tile buffers, each: pre [pixel 256][64], then dyt [co 3][row 10][col 40]
    double* scratch = reinterpret_cast<double*>(lds + 2 * TB_BUF);                  // (70336 = 8 x 8792: aligned)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, kk = lane >> 5;
    const int w4 = wave & 3;                   // the wave's pair of tile rows: 2 w4, 2 w4 + 1
    const bool dgw = wave >= 4;                // waves 0-3: weight gradient; waves 4-7: data gradient, slope term, store of g
    const bool hth = tid < 256;                // the gradient halo and the bias partials stay on wgrad_toimage_f32_kernel's 256 threads
    const float slope = a.slope_p ? a.slope_p[0] : a.slope;

    // ---- weight gradient, B column n = (ky', kx', co): halo row r + ky', halo column x + kx' + 3 ----------------------------
    int bbase;
    {
        const int nn = l31 < 27 ? l31 : 0;
        const int kyf = nn / 9, kxf = (nn - 9 * kyf) / 3, co = nn - 9 * kyf - 3 * kxf;
        bbase = (co * TB_GROWS + kyf) * TB_GW + kxf + 3 + kk;
    }
    // ---- data gradient, K slot 2 s + kk = 10 (2 - ky) + 3 (2 - kx) + co (slot 9 of every ten: zero): the lane's pixel column
    // l31 reads dyt at halo (r + 2 - ky, l31 + 5 - kx); its channel 32 mh + l31 multiplies W[co][ci][ky][kx] --------------------
    int koff[TB_KSTEPS];
    float wd[2][TB_KSTEPS];
#pragma unroll
    for (int s = 0; s < TB_KSTEPS; ++s) {
        const int kq = 2 * s + kk, rp = kq / 10, j = kq - 10 * rp;
        const bool tap_ok = j < 9;
        const int jj = tap_ok ? j : 0, sp = jj / 3, co = jj - 3 * sp, ky = 2 - rp, kx = 2 - sp;
        koff[s] = (co * TB_GROWS + 2 - ky) * TB_GW + 5 - kx + l31;
#pragma unroll
        for (int mh = 0; mh < 2; ++mh) {
            const int ci = 32 * mh + l31, chunk = ci / a.w_CK, cl = ci - chunk * a.w_CK;
            const float w = a.wpk[((chunk * 3 + ky) * a.w_CoutPad + co) * a.w_KROWP + kx * a.w_PS + cl];
            wd[mh][s] = tap_ok ? w : 0.f;
        }
    }

    // ---- staging ---------------------------------------------------------------------------------------------------------------
    const unsigned plane = (unsigned)(a.H * a.W);
    const __amdgpu_buffer_rsrc_t rg = sisr_rsrc(a.g1, (unsigned)a.N * 3u * plane * 4u),
                                 ry = sisr_rsrc(TANHB ? a.g2 : a.g1, (unsigned)a.N * 3u * plane * 4u);
    const __amdgpu_buffer_rsrc_t rx = sisr_rsrc(a.pre, (unsigned)a.N * plane * 256u);
    const __amdgpu_buffer_rsrc_t ro = sisr_rsrc(a.g, (unsigned)a.N * plane * 256u);
    // pre: item i of a thread = 16-byte group (tid + 512 i): pixel = group / 16, channels 4 (group % 16) ..
    // gradient halo (threads < 256): element (tid + 256 k) of [co][row][col]
    int g_co[TB_GITEMS], g_row[TB_GITEMS], g_col[TB_GITEMS];
#pragma unroll
    for (int k = 0; k < TB_GITEMS; ++k) {
        const int idx = (tid & 255) + 256 * k;
        g_co[k] = idx / (TB_GROWS * TB_GW);
        const int rem = idx - g_co[k] * (TB_GROWS * TB_GW);
        g_row[k] = rem / TB_GW;
        g_col[k] = rem - g_row[k] * TB_GW;
    }
    f32x4 sx[TB_XITEMS];
    float sg[TB_GITEMS], sy[TB_GITEMS];
    float bsum[3] = {0.f, 0.f, 0.f};
    double dsl = 0.0;

    auto issue = [&](int T) {
        const int n = T / a.per_img, r = T - n * a.per_img;
        const int ty = r / a.tiles_x, tx = r - ty * a.tiles_x;
        const int live = T < a.total;
        // (an out-of-range item gets offset 2^31 and is dropped by the buffer unit: zeros = the convolution's padding)
#pragma unroll
        for (int k = 0; k < TB_GITEMS; ++k) {
            const int Y = ty * TB_TH - 1 + g_row[k], X = tx * TB_TW - 4 + g_col[k];
            const int ok = live & (int)hth & (int)(g_co[k] < 3) & (int)((unsigned)Y < (unsigned)a.H) & (int)((unsigned)X < (unsigned)a.W);
            const unsigned voff = ok ? (unsigned)((((n * 3 + g_co[k]) * a.H + Y) * a.W + X) * 4) : 0x80000000u;
            sg[k] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rg, voff, 0, 0));
            if (TANHB) sy[k] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ry, voff, 0, 0));
        }
        const int origin = ((n * a.H + ty * TB_TH) * a.W + tx * TB_TW) * 256;
#pragma unroll
        for (int i = 0; i < TB_XITEMS; ++i) {
            const int grp = tid + TB_THREADS * i, p = grp >> 4, c4 = grp & 15;
            const unsigned voff = live ? (unsigned)(origin + ((p >> 5) * a.W + (p & 31)) * 256 + c4 * 16) : 0x80000000u;
            sx[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rx, voff, 0, 0));
        }
    };
    auto commit = [&](int buf) {
        float* xs = reinterpret_cast<float*>(lds + buf * TB_BUF);
        float* gs = reinterpret_cast<float*>(lds + buf * TB_BUF + TB_XBYTES);
#pragma unroll
        for (int k = 0; k < TB_GITEMS; ++k) {
            const float e = TANHB ? sg[k] * (1.f - sy[k] * sy[k]) : sg[k];
            if (hth && g_co[k] < 3) gs[tid + 256 * k] = e;
            // bias partial: the tile's own pixels = halo rows 1 .. 8, halo columns 4 .. 35
            const bool mine = hth && g_row[k] >= 1 && g_row[k] <= TB_TH && g_col[k] >= 4 && g_col[k] < 4 + TB_TW;
#pragma unroll
            for (int c = 0; c < 3; ++c) bsum[c] += (mine && g_co[k] == c) ? e : 0.f;
        }
#pragma unroll
        for (int i = 0; i < TB_XITEMS; ++i)
            *reinterpret_cast<f32x4*>(xs + (tid + TB_THREADS * i) * 4) = sx[i];      // [pixel][64]: group index = pixel * 16 + c4
    };

    f32x16 acc[2];
#pragma unroll
    for (int mh = 0; mh < 2; ++mh)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[mh][i] = 0.f;

    // tile T is contracted out of buffer `buf` while tile T + grid, whose loads were issued a whole tile earlier, is committed to
    // the other buffer (no wave reads it: ONE barrier per tile) and tile T + 2 grid is requested: loads are in flight all the time
    int T = blockIdx.x, buf = 0;
    issue(T);
    commit(0);
    issue(T + gridDim.x);
    __syncthreads();
    for (; T < a.total; T += gridDim.x, buf ^= 1) {
        const float* xs = reinterpret_cast<const float*>(lds + buf * TB_BUF);
        const float* gs = reinterpret_cast<const float*>(lds + buf * TB_BUF + TB_XBYTES);
        if (!dgw) {
            // ---- weight gradient: pixels (r, 2 sxp + kk) ----------------------------------------------------------------------
#pragma unroll
            for (int rr = 0; rr < 2; ++rr) {
                const int r = 2 * w4 + rr;
#pragma unroll
                for (int sxp = 0; sxp < 16; ++sxp) {
                    const float* xp = xs + (r * TB_TW + 2 * sxp + kk) * TB_PS + l31;
                    const float b = gs[bbase + r * TB_GW + 2 * sxp];
                    acc[0] = mfma32(lrelu(xp[0], slope), b, acc[0]);
                    acc[1] = mfma32(lrelu(xp[32], slope), b, acc[1]);
                }
            }
            commit(buf ^ 1);
            issue(T + 2 * gridDim.x);
        } else {
            commit(buf ^ 1);
            issue(T + 2 * gridDim.x);
            const int n = T / a.per_img, rem = T - n * a.per_img;
            const int ty = rem / a.tiles_x, tx = rem - ty * a.tiles_x;
            const int origin = ((n * a.H + ty * TB_TH) * a.W + tx * TB_TW) * 256;   // byte offset of the tile in pre and in g
            // ---- data gradient of tile row r, the slope term and the store of g -----------------------------------------------
#pragma unroll
            for (int rr = 0; rr < 2; ++rr) {
                const int r = 2 * w4 + rr;
                f32x16 dacc[2];
#pragma unroll
                for (int mh = 0; mh < 2; ++mh)
#pragma unroll
                    for (int i = 0; i < 16; ++i) dacc[mh][i] = 0.f;
#pragma unroll
                for (int s = 0; s < TB_KSTEPS; ++s) {
                    float av = gs[koff[s] + r * TB_GW];
                    if (s % 5 == 4) av = kk ? 0.f : av;                         // the zero slot of a tap row
                    dacc[0] = mfma32(av, wd[0][s], dacc[0]);
                    dacc[1] = mfma32(av, wd[1][s], dacc[1]);
                }
#pragma unroll
                for (int mh = 0; mh < 2; ++mh)
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int px = mfma_row(i, lane);                       // accumulator row = pixel column of the tile
                        const float pv = xs[(r * TB_TW + px) * TB_PS + 32 * mh + l31], gv = dacc[mh][i];
                        if (!(pv > 0.f)) dsl += (double)gv * (double)pv;
                        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, gv), ro,
                                                              (unsigned)(origin + (r * a.W + px) * 256 + (32 * mh + l31) * 4), 0, 0);
                    }
            }
        }
        __syncthreads();          // every wave has finished reading this tile and committed its share of the next one
    }

    // ---- slope partial of the workgroup: lanes, then the four data-gradient waves, in a fixed order ----------------------------
    dsl = wave_sum(dsl);
    if (lane == 0) scratch[wave] = dsl;
    __syncthreads();
    if (tid == 0) a.dslope_part[blockIdx.x] = (scratch[4] + scratch[5]) + (scratch[6] + scratch[7]);
    // ---- the four waves' partial D[ci][n] meet in LDS; then every entry of the slab is written (wgrad_toimage_f32_kernel's) ----
    float* part = reinterpret_cast<float*>(lds);                  // [wave][ci 64][n 32]
    float* bred = part + 4 * 64 * 32;                              // [256][3] bias partials
    if (!dgw) {
#pragma unroll
        for (int mh = 0; mh < 2; ++mh)
#pragma unroll
            for (int i = 0; i < 16; ++i) part[(wave * 64 + 32 * mh + mfma_row(i, lane)) * 32 + l31] = acc[mh][i];
#pragma unroll
        for (int c = 0; c < 3; ++c) bred[tid * 3 + c] = bsum[c];
    }
    __syncthreads();
    // slab element idx = ((chunk * 3 + ky) * KROWP + krow) * CoutPad + co, krow = kx * PS + cl; a thread walks idx = tid, tid + 512, ..
    // with carries instead of divisions
    float* sl = a.slab + (long long)blockIdx.x * a.slab_stride;
    const int dco = TB_THREADS % a.CoutPad, dt = TB_THREADS / a.CoutPad, dkrow = dt % a.KROWP, dt2 = dt / a.KROWP;
    int co = tid % a.CoutPad, t = tid / a.CoutPad, krow = t % a.KROWP, t2 = t / a.KROWP;
    for (int idx = tid; idx < a.slab_elems; idx += TB_THREADS) {
        const int ky = t2 % 3, chunk = t2 / 3;
        const int kx = (int)(krow >= a.PS) + (int)(krow >= 2 * a.PS) + (int)(krow >= 3 * a.PS), cl = krow - kx * a.PS;
        float v = 0.f;
        if (co < 3 && kx < 3 && cl < a.CK) {
            const int n = (2 - ky) * 9 + (2 - kx) * 3 + co, ci = chunk * a.CK + cl;
#pragma unroll
            for (int w = 0; w < 4; ++w) v += part[(w * 64 + ci) * 32 + n];
        }
        sl[idx] = v;
        co += dco;
        const int c1 = co >= a.CoutPad;
        co -= c1 ? a.CoutPad : 0;
        krow += dkrow + c1;
        const int c2 = krow >= a.KROWP;
        krow -= c2 ? a.KROWP : 0;
        t2 += dt2 + c2;
    }
    if (a.bias_slab != nullptr && tid < a.CoutPad) {
        float s = 0.f;
        if (tid < 3)
            for (int i = 0; i < 256; ++i) s += bred[i * 3 + tid];
        a.bias_slab[(long long)blockIdx.x * a.slab_stride + tid] = s;
    }
}

// dslope[0] = the sum of the n (<= 256 x 4) workgroup partials: thread t adds partials t, t + 256, ..., then lanes and waves in order
__global__ void __launch_bounds__(SISR_BLOCK) toimage_bwd_finish_kernel(const double* __restrict__ part, int n, float* __restrict__ out) {
    __shared__ double scratch[SISR_BLOCK / 64];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += SISR_BLOCK) s += part[i];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) out[0] = (float)((scratch[0] + scratch[1]) + (scratch[2] + scratch[3]));
}

extern "C" int sisr_toimage_bwd_f32_eligible(const SisrToImageBwdDesc* d) {
    // A/B switches: SISR_TOIMAGE_BWD=0 keeps the three separate kernels; SISR_THIN=0 keeps the generic kernels for them
    if (sisr_switch_off("SISR_TOIMAGE_BWD") || sisr_switch_off("SISR_THIN") || !d) return 0;
    if (d->KH != 3 || d->KW != 3 || d->stride != 1 || d->pad_y != 1 || d->pad_x != 1) return 0;
    if (d->Cin != 64 || d->Cout != 3 || d->pre_bf16 || d->g_bf16) return 0;
    if (d->N < 1 || d->H < 1 || d->W < 1 || (d->H % TB_TH) || (d->W % TB_TW)) return 0;
    if ((int64_t)d->N * d->H * d->W * 256 >= (1ll << 31)) return 0;
    // the slab, as sisr_wgrad_plan lays it out: [chunk][ky][kx * PS + cl][CoutPad]
    if (d->CoutPad < 3 || d->CoutPad > 256 || d->CK < 1 || d->n_chunk * d->CK != 64) return 0;
    if (d->PS < d->CK || d->KROWP < 2 * d->PS + d->CK || d->slab_elems != d->n_chunk * 3 * d->KROWP * d->CoutPad) return 0;
    if (d->slab_stride < d->slab_elems) return 0;
    // the forward weight image, as sisr_conv2d_plan lays it out: [chunk][ky][cout][kx * PS + cl]
    if (d->w_CK < 1 || (64 % d->w_CK) || d->w_PS < d->w_CK || d->w_KROWP < 2 * d->w_PS + d->w_CK || d->w_CoutPad < 3) return 0;
    return 1;
}

extern "C" int sisr_toimage_bwd_f32_parts(const SisrToImageBwdDesc* d) {
    if (!d || d->H < TB_TH || d->W < TB_TW || d->N < 1) return SISR_E_BADARG;
    return sisr_equal_shares(d->N * (d->H / TB_TH) * (d->W / TB_TW), sisr_cu_slots());      // (= sisr_wgrad_toimage_slabs)
}

extern "C" int sisr_toimage_bwd_desc_bytes(void) { return (int)sizeof(SisrToImageBwdDesc); }

extern "C" int sisr_toimage_bwd_f32(const SisrToImageBwdDesc* d, void* stream) {
    if (!d || !d->pre || !d->dy || !d->wpk || !d->g || !d->slab || !d->dslope_part || !d->dslope) return SISR_E_BADARG;
    if (reinterpret_cast<uintptr_t>(d->dslope_part) & 7) return SISR_E_BADARG;
    if (sisr_toimage_bwd_f32_eligible(d) != 1) return SISR_E_UNSUPPORTED;
    ToImageBwdArgs a;
    a.pre = d->pre; a.g1 = d->dy; a.g2 = d->out; a.wpk = d->wpk;
    a.g = d->g; a.slab = d->slab; a.bias_slab = d->bias_slab; a.dslope_part = reinterpret_cast<double*>(d->dslope_part);
    a.slope_p = d->slope_p; a.slope = d->slope;
    a.N = d->N; a.H = d->H; a.W = d->W;
    a.tiles_x = d->W / TB_TW;
    a.per_img = a.tiles_x * (d->H / TB_TH);
    a.total = a.per_img * d->N;
    a.w_CK = d->w_CK; a.w_PS = d->w_PS; a.w_KROWP = d->w_KROWP; a.w_CoutPad = d->w_CoutPad;
    a.CK = d->CK; a.PS = d->PS; a.KROWP = d->KROWP; a.CoutPad = d->CoutPad; a.slab_elems = d->slab_elems;
    a.slab_stride = d->slab_stride;
    const int grid = sisr_toimage_bwd_f32_parts(d);
    constexpr int lds_bytes = 2 * TB_BUF + 64;
    const hipStream_t st = sisr_stream(stream);
    const int e = d->out ? sisr_launch<toimage_bwd_f32_kernel<true>>(dim3(grid), dim3(TB_THREADS), lds_bytes, 0, st, a)
                         : sisr_launch<toimage_bwd_f32_kernel<false>>(dim3(grid), dim3(TB_THREADS), lds_bytes, 0, st, a);
    if (e) return e;
    hipLaunchKernelGGL(toimage_bwd_finish_kernel, dim3(1), dim3(SISR_BLOCK), 0, st, a.dslope_part, grid, d->dslope);
    SISR_CHECK_LAUNCH();
    return 0;
}
