// spectral.hip -- weight-side kernels: spectral-norm power iteration, weight packing for the
// direct-conv kernels, and the weight-gradient epilogue (un-packing + spectral-norm quotient rule).
//
// Restates torch.nn.utils.spectral_norm's hook (SpectralNorm.compute_weight), which the reference
// applies to every trunk convolution of G and every convolution of D (model_generator.py:3,10,13,
// 33,39,45,52,123; model_discriminator.py:2,10,39):
//   training: v <- normalize(W_mat^T u), u <- normalize(W_mat v)  (one iteration, eps 1e-12, in place)
//   sigma = u . (W_mat v);  W = W_orig / sigma;  autograd treats u, v as constants.
// "Multi-tensor": one launch serves every convolution of a network (descriptor table in HBM).
#include "sisr_dev.h"

#include <algorithm>

#include "sisr_bf16_stage.h"

#define SN_EPS 1e-12f

// Power iteration in four short multi-tensor launches (grid = (weights, jobs); surplus workgroups exit), so
// the 512x4608 matrices of the discriminator are spread over the chip instead of one workgroup per matrix:
//   A  t_part[rb][j] = sum_{i in row block rb} W[i][j] u[i]        (workgroup = 16 rows x 1024 columns)
//   B  t = sum_rb t_part                                           (thread per column)
//   C  s'[i] = W[i,:] . t                                          (wave per row, 4 rows per workgroup)
//   D  v = t / max(|t|, eps) ; s = s' / max(|t|, eps) ; u = s / max(|s|, eps) ; sigma = u . s   (one workgroup per weight)
// Evaluation mode skips A/B (C uses the stored v) and D keeps the stored u.  sn_work per weight: [RB][cols] + [rows] floats.
#define SN_RB 16
#define SN_CB 1024
__device__ __forceinline__ int sn_rblocks(int rows) { return (rows + SN_RB - 1) / SN_RB; }

__global__ void __launch_bounds__(SISR_BLOCK) sn_wt_u_kernel(const SisrWeightDesc* table) {
    __shared__ float us[SN_RB];
    const SisrWeightDesc w = table[blockIdx.x];
    if (w.u == nullptr || !w.training) return;
    const int rows = w.Cout, cols = w.Cin * w.KH * w.KW;
    const int ncb = (cols + SN_CB - 1) / SN_CB, job = blockIdx.y;
    if (job >= sn_rblocks(rows) * ncb) return;
    const int rb = job / ncb, cb = job - rb * ncb;
    const int r0 = rb * SN_RB, nr = min(SN_RB, rows - r0);
    if (threadIdx.x < nr) us[threadIdx.x] = w.u[r0 + threadIdx.x];
    __syncthreads();
    if ((cols & 3) == 0 && nr == SN_RB) {
        // whole row block, rows of whole float4s: a thread owns four consecutive columns and has all 16 rows' loads in flight at
        // once (the scalar loop below waits for each row before it asks for the next: the phase was latency-bound at 31 us)
        const int j = cb * SN_CB + threadIdx.x * 4;
        if (j >= cols) return;
        const float* wp = w.w_orig + (int64_t)r0 * cols + j;
        f32x4 v[SN_RB];
#pragma unroll
        for (int i = 0; i < SN_RB; ++i) v[i] = *reinterpret_cast<const f32x4*>(wp + (int64_t)i * cols);
        f32x4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < SN_RB; ++i) a += v[i] * us[i];             // row order, as the scalar path: same bits
        *reinterpret_cast<f32x4*>(w.sn_work + (int64_t)rb * cols + j) = a;
        return;
    }
    float acc[SN_CB / SISR_BLOCK];
#pragma unroll
    for (int k = 0; k < SN_CB / SISR_BLOCK; ++k) acc[k] = 0.f;
    const int j0 = cb * SN_CB + threadIdx.x;
    const float* wp = w.w_orig + (int64_t)r0 * cols;
    for (int i = 0; i < nr; ++i, wp += cols) {
        const float ui = us[i];
#pragma unroll
        for (int k = 0; k < SN_CB / SISR_BLOCK; ++k) {
            const int j = j0 + k * SISR_BLOCK;
            if (j < cols) acc[k] += wp[j] * ui;
        }
    }
#pragma unroll
    for (int k = 0; k < SN_CB / SISR_BLOCK; ++k) {
        const int j = j0 + k * SISR_BLOCK;
        if (j < cols) w.sn_work[(int64_t)rb * cols + j] = acc[k];
    }
}

__global__ void __launch_bounds__(SISR_BLOCK) sn_t_sum_kernel(const SisrWeightDesc* table) {
    const SisrWeightDesc w = table[blockIdx.x];
    if (w.u == nullptr || !w.training) return;
    const int rows = w.Cout, cols = w.Cin * w.KH * w.KW;
    const int j = blockIdx.y * SISR_BLOCK + threadIdx.x;
    if (j >= cols) return;
    const int nrb = sn_rblocks(rows);
    float t = 0.f;
    for (int rb = 0; rb < nrb; ++rb) t += w.sn_work[(int64_t)rb * cols + j];
    w.sn_work[j] = t;                                   // row block 0 now holds t = W^T u (not yet normalised)
}

// s' = W t (training; the 1/|t| factor is applied by the finishing kernel) or s = W v (evaluation)
__global__ void __launch_bounds__(SISR_BLOCK) sn_w_v_kernel(const SisrWeightDesc* table) {
    const SisrWeightDesc w = table[blockIdx.x];
    if (w.u == nullptr) return;
    const int rows = w.Cout, cols = w.Cin * w.KH * w.KW;
    const int lane = threadIdx.x & 63, i = blockIdx.y * (SISR_BLOCK / 64) + (threadIdx.x >> 6);
    if (i >= rows) return;
    const float* wr = w.w_orig + (int64_t)i * cols;
    const float* vec = w.training ? w.sn_work : w.v;
    float a = 0.f;
    // twelve loads of each operand in flight per round; the adds keep the order of the plain loop (j = lane, lane + 64, ...), so the
    // result is bit-identical to it (the plain loop waited for every load before asking for the next: 72 dependent rounds for the
    // discriminator's 4,608 columns)
    for (int j0 = lane; j0 < cols; j0 += 64 * 12) {
        float wv[12], vv[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) {
            const int jj = min(j0 + 64 * k, cols - 1);
            wv[k] = wr[jj]; vv[k] = vec[jj];
        }
#pragma unroll
        for (int k = 0; k < 12; ++k)
            if (j0 + 64 * k < cols) a += wv[k] * vv[k];
    }
    a = wave_sum(a);
    if (lane == 0) w.sn_work[(int64_t)sn_rblocks(rows) * cols + i] = a;
}

__global__ void __launch_bounds__(SISR_BLOCK) sn_u_finish_kernel(const SisrWeightDesc* table) {
    __shared__ float scratch[8];
    const SisrWeightDesc w = table[blockIdx.x];
    const int tid = threadIdx.x;
    if (w.u == nullptr) {
        if (tid == 0 && w.sigma) { w.sigma[0] = 1.f; w.sigma[1] = 1.f; }
        return;
    }
    const int rows = w.Cout, cols = w.Cin * w.KH * w.KW;
    const float* s = w.sn_work + (int64_t)sn_rblocks(rows) * cols;
    float iv = 1.f, iu = 0.f;
    if (w.training) {
        // v = t / max(|t|, eps) ; s = W v = s' / max(|t|, eps) ; u = s / max(|s|, eps)
        float part = 0.f;
        for (int j = tid; j < cols; j += SISR_BLOCK) part += w.sn_work[j] * w.sn_work[j];
        iv = 1.f / fmaxf(sqrtf(block_sum(part, scratch)), SN_EPS);
        for (int j = tid; j < cols; j += SISR_BLOCK) {
            const float v = w.sn_work[j] * iv;
            w.v[j] = v;
            if (w.v_used) w.v_used[j] = v;
        }
        part = 0.f;
        for (int i = tid; i < rows; i += SISR_BLOCK) { const float si = s[i] * iv; part += si * si; }
        iu = 1.f / fmaxf(sqrtf(block_sum(part, scratch)), SN_EPS);
    } else if (w.v_used) {
        for (int j = tid; j < cols; j += SISR_BLOCK) w.v_used[j] = w.v[j];
    }
    float part = 0.f;
    for (int i = tid; i < rows; i += SISR_BLOCK) {
        const float si = s[i] * iv;
        const float u = w.training ? si * iu : w.u[i];
        part += u * si;
        if (w.training) w.u[i] = u;
        if (w.u_used) w.u_used[i] = u;
    }
    const float sigma = block_sum(part, scratch);
    if (tid == 0 && w.sigma) { w.sigma[0] = sigma; w.sigma[1] = 1.f / sigma; }      // [1]: the conv_deep.hip epilogue scale
}

// packed channel index -> original output channel (PixelShuffle(2) consumers use (i,j)-major order)
__device__ __forceinline__ int unpermute_cout(int cp, int Cout, int shuffle2) {
    if (!shuffle2) return cp;
    const int Cq = Cout >> 2;
    const int ij = cp / Cq, c = cp - ij * Cq;
    return c * 4 + ij;
}

// elements of an image's standard order (fp32 words for SISR_WIMG_F32, bf16 otherwise); the formats: include/sisr_hip.h
__host__ __device__ __forceinline__ int64_t wimg_elems(const SisrWeightImage& g) {
    if (g.format == SISR_WIMG_F32) return (int64_t)g.n_chunk * g.KH * g.CoutPad * g.KROWP;
    if (g.format == SISR_WIMG_BF16) return (int64_t)g.n_chunk * g.CoutPad * g.KH * g.KW * g.CK;
    return (int64_t)g.n_chunk * g.KH * g.CoutPad * (g.extra * 32 + 8);
}
// bytes of the image with the copy `extra` asks for behind it: the one place that knows an image's size
__host__ __device__ __forceinline__ int64_t wimg_bytes(const SisrWeightImage& g) {
    if (g.format == SISR_WIMG_F32) return 4 * (wimg_elems(g) + (g.extra ? SISR_WLDS_WORDS : 0));
    return 2 * wimg_elems(g) * (g.format == SISR_WIMG_BF16 && g.extra ? 2 : 1);
}

// what every image of a weight is gathered from (the kernels copy it out of the table once; the image records follow one by one)
struct WimgSource {
    const float* w_orig;
    int Cout, Cin, KH, KW, shuffle2;
    float inv;                                                         // 1 / sigma
};
// THE read of W_orig: element (out channel o, in channel i, tap (rp, sp)) of image g = forward tap (R0y + Sy rp, R0x + Sx sp) of
// W_orig times inv, zero for a channel or a tap outside the weight (a tap past the image's own KH x KW maps outside the weight
// under every tap map in use).  One predicate of unsigned compares (a negative tap is a huge one) and a 32-bit index -- a weight
// is far below 2^31 elements -- keep the per-element cost at that of a hard-wired map: the pack kernels are bound by it.
__device__ __forceinline__ float wimg_value(const WimgSource& w, const SisrWeightImage& g, unsigned o, unsigned i, int rp, int sp) {
    const unsigned cp = g.transposed ? i : o, ci = g.transposed ? o : i;      // packed forward cout, forward cin
    const unsigned r = (unsigned)(g.R0y + g.Sy * rp), s = (unsigned)(g.R0x + g.Sx * sp);
    if ((cp >= (unsigned)w.Cout) | (ci >= (unsigned)w.Cin) | (r >= (unsigned)w.KH) | (s >= (unsigned)w.KW)) return 0.f;
    const unsigned co = (unsigned)unpermute_cout((int)cp, w.Cout, w.shuffle2);
    return w.w_orig[((co * (unsigned)w.Cin + ci) * (unsigned)w.KH + r) * (unsigned)w.KW + s] * w.inv;
}

// phase 2: pack W/sigma.  grid (n_weights, parts); a workgroup walks the images of its weight, grid-stride over the elements of
// each: one loop per storage order.  (Packed images are far below 2^32 elements: 32-bit index arithmetic.)
// (The descriptor is copied by value and the image loop unrolled, so that every field of every record is fetched in ONE batch of
// scalar loads before the first store: a workgroup has only a few elements of each image to hide a dependent round trip per
// record behind.)
__global__ void __launch_bounds__(SISR_BLOCK) weights_pack_kernel(const SisrWeightDesc* table) {
    const SisrWeightDesc t = table[blockIdx.x];
    const WimgSource w = {t.w_orig, t.Cout, t.Cin, t.KH, t.KW, t.shuffle2, 1.f / (t.sigma ? t.sigma[0] : 1.f)};
    const int64_t stride = (int64_t)gridDim.y * SISR_BLOCK;
    const int64_t start = (int64_t)blockIdx.y * SISR_BLOCK + threadIdx.x;
#pragma unroll
    for (int gi = 0; gi < SISR_WEIGHT_IMAGES; ++gi) {
        const SisrWeightImage& g = t.img[gi];
        if (g.dst == nullptr || g.format == SISR_WIMG_DEEP) continue;
        const int64_t total = wimg_elems(g);
        if (g.format == SISR_WIMG_F32) {
            float* dst = reinterpret_cast<float*>(g.dst);
            for (int64_t e = start; e < total; e += stride) {           // [chunk][r'][out][krow], krow = s' * PS + (in - chunk * CK)
                unsigned tq = (unsigned)e;
                const unsigned krow = tq % g.KROWP; tq /= g.KROWP;
                const unsigned o = tq % g.CoutPad; tq /= g.CoutPad;
                const unsigned rp = tq % g.KH, chunk = tq / g.KH;
                const unsigned sp = krow / g.PS, il = krow - sp * g.PS;
                dst[e] = il < (unsigned)g.CK ? wimg_value(w, g, o, chunk * g.CK + il, rp, sp) : 0.f;
            }
            if (g.extra == 0) continue;
            // the fp32-tensor trunk conv's LDS order, behind the standard image: the same numbers
            unsigned* lds = reinterpret_cast<unsigned*>(dst + total);
            for (int64_t e = start; e < SISR_WLDS_WORDS; e += stride) {
                unsigned tq = (unsigned)e;
                const unsigned wd = tq % 36u; tq /= 36u;
                const unsigned oc = tq & 31u; tq >>= 5;
                const unsigned tap = tq % 9u; tq /= 9u;
                const unsigned q = tq & 1u, o = 32 * (tq >> 1) + oc;
                const unsigned rp = tap / 3, sp = tap - 3 * rp;
                unsigned word = 0u;
                if (wd < 32 && g.extra == 1) {
                    word = __float_as_uint(wimg_value(w, g, o, 32 * q + wd, rp, sp));
                } else if (wd < 32) {
                    const unsigned m = wd & 15;
                    const float v0 = wimg_value(w, g, o, 32 * q + 2 * m, rp, sp), v1 = wimg_value(w, g, o, 32 * q + 2 * m + 1, rp, sp);
                    const __bf16 h0 = (__bf16)v0, h1 = (__bf16)v1;
                    if (wd < 16) {
                        word = (unsigned)__builtin_bit_cast(unsigned short, h0) | ((unsigned)__builtin_bit_cast(unsigned short, h1) << 16);
                    } else {
                        const __bf16 l0 = (__bf16)(v0 - (float)h0), l1 = (__bf16)(v1 - (float)h1);
                        word = (unsigned)__builtin_bit_cast(unsigned short, l0) | ((unsigned)__builtin_bit_cast(unsigned short, l1) << 16);
                    }
                }
                lds[e] = word;
            }
        } else {
            __bf16* dst = reinterpret_cast<__bf16*>(g.dst);
            const unsigned WSG = g.KH * g.KW * g.CK;
            for (int64_t e = start; e < total; e += stride) {           // [chunk][out][tap * CK + (in - chunk * CK)]
                unsigned tq = (unsigned)e;
                const unsigned kidx = tq % WSG; tq /= WSG;
                const unsigned o = tq % g.CoutPad, chunk = tq / g.CoutPad;
                const unsigned tap = kidx / g.CK, il = kidx - tap * g.CK;
                const unsigned rp = tap / g.KW, sp = tap - rp * g.KW;
                dst[e] = (__bf16)wimg_value(w, g, o, chunk * g.CK + il, rp, sp);
            }
            if (g.extra == 0) continue;
            // the same values in the persistent trunk kernels' load order, behind the standard image
            for (int64_t e = start; e < total; e += stride) {
                unsigned tq = (unsigned)e;
                const unsigned el = tq & 7; tq >>= 3;
                const unsigned lane = tq & 63; tq >>= 6;
                const unsigned j = tq & 3; tq >>= 2;
                const unsigned tap = tq % 9;
                const unsigned o = tq / 9 * 32 + (lane & 31);
                const unsigned i = (j >> 1) * 32 + (j & 1) * 16 + 8 * (lane >> 5) + el;
                const unsigned rp = tap / g.KW, sp = tap - rp * g.KW;
                dst[total + e] = (__bf16)wimg_value(w, g, o, i, rp, sp);
            }
        }
    }
}

// the rows of image g that the workgroup's tile (cout chunk cb, cin chunk kb, in `tile`) holds, in 16-byte items of 8 bf16: 8
// consecutive in-channels of one tap column (or the 8 padding slots).  TR is g.transposed as a constant: the LDS strides become
// instruction offsets, and this loop's time goes to its instructions.
template <bool TR>
__device__ __forceinline__ void wimg_deep_rows(const SisrWeightImage& g, const float* tile, int cb, int kb, int Cout, int Cin) {
    __bf16* dst = reinterpret_cast<__bf16*>(g.dst);
    const int RW = g.extra * 32 + 8, G8 = RW >> 3;
    // this tile in the image's view: out block / in block, and where (out oc, in ic) sits in `tile`
    const int ob = TR ? kb : cb, ib = TR ? cb : kb, n_out = TR ? Cin : Cout;
    constexpr int so = TR ? 9 : 289, si = TR ? 289 : 9;
    for (int i = threadIdx.x; i < g.KH * 32 * G8; i += SISR_BLOCK) {
        const int row = i / G8, k8 = i - row * G8, rp = row >> 5, oc = row & 31, sp = k8 >> 2;
        const unsigned r = g.R0y + g.Sy * rp, sx = g.R0x + g.Sx * sp;         // (a negative tap is a huge one)
        const bool ok = (sp < g.KW) & (r < 3u) & (sx < 3u);
        const float* src = tile + oc * so + (k8 & 3) * 8 * si + (ok ? r * 3 + sx : 0u);
        float v[8];                                                    // (read for a zero item too: its address is inside the tile)
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = src[j * si];
        const u32x4 q = {pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7])};
        *reinterpret_cast<u32x4*>(dst + ((unsigned)((ib * g.KH + rp) * n_out + ob * 32 + oc) * RW + k8 * 8)) =
            ok ? q : u32x4{0u, 0u, 0u, 0u};
    }
}

// conv_deep.hip images (SISR_WIMG_DEEP): [32-channel chunk][tap row][out][taps per row * 32 + 8] bf16, element s' * 32 + in, the
// taps a row has no s' for and its 8 padding elements zero.  Workgroup = one 32 cout x 32 cin tile of a 3x3 weight: its 32 x 288
// floats are read ONCE, as 32 contiguous 1,152-byte pieces (the generic pack kernel gathers every element with a 36-byte stride,
// once per image), pass through LDS and leave as whole rows of every image that is asked for -- forward, data gradient (channels
// swapped, taps flipped), the four output-parity classes of a stride-2 layer's data gradient.  grid (weights, cout chunks, cin chunks).
__global__ void __launch_bounds__(SISR_BLOCK) weights_pack_deep_kernel(const SisrWeightDesc* table) {
    __shared__ float tile[32 * (9 * 32 + 1)];                      // [cout][ci * 9 + tap], rows of 289
    // most workgroups of the grid (sized for the largest weight) lie outside their weight: they leave on its dims alone, before
    // the records are copied
    const SisrWeightDesc& t = table[blockIdx.x];
    const int cb = blockIdx.y, kb = blockIdx.z;                    // cout chunk, cin chunk
    if ((cb * 32 >= t.Cout) | (kb * 32 >= t.Cin) | (t.KH != 3) | (t.KW != 3)) return;
    const SisrWeightDesc w = t;                                    // (by value, image loops unrolled: see weights_pack_kernel)
    bool any = false;
#pragma unroll
    for (int gi = 0; gi < SISR_WEIGHT_IMAGES; ++gi) any |= w.img[gi].dst != nullptr && w.img[gi].format == SISR_WIMG_DEEP;
    if (!any) return;
    const int Cout = w.Cout, Cin = w.Cin;
    const float* sigma = w.wdp_scaled ? w.sigma : nullptr;         // (a select: the pointer comes with the records' batch)
    const float sc = sigma ? 1.f / sigma[0] : 1.f;
    const int tid = threadIdx.x;
    // 32 couts x 288 contiguous floats (32 ci x 9 taps; 1,152-byte rows: 16-byte aligned), one float4 per item
    const float* w_orig = w.w_orig;
    for (int i = tid; i < 32 * 72; i += SISR_BLOCK) {
        const int co = i / 72, e4 = i - co * 72;
        const f32x4 v = *reinterpret_cast<const f32x4*>(w_orig + ((int64_t)(cb * 32 + co) * Cin + kb * 32) * 9 + e4 * 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) tile[co * 289 + e4 * 4 + j] = v[j] * sc;
    }
    __syncthreads();
#pragma unroll
    for (int gi = 0; gi < SISR_WEIGHT_IMAGES; ++gi) {
        const SisrWeightImage& g = w.img[gi];
        if (g.dst == nullptr || g.format != SISR_WIMG_DEEP) continue;
        g.transposed ? wimg_deep_rows<true>(g, tile, cb, kb, Cout, Cin) : wimg_deep_rows<false>(g, tile, cb, kb, Cout, Cin);
    }
}

// weight-gradient epilogue: the reduced packed gradient is a [K rows][CoutPad] matrix (K = chunk, tap, channel
// in the conv kernels' order), the parameter gradient is OIHW -- a transpose with a row permutation.  A workgroup
// takes one tile (32 packed couts x one channel chunk x all taps) through LDS: coalesced 128-byte reads along the
// couts, contiguous writes along (ci, r, s).  Two launches over grid (weights, max tiles per weight):
//   1. partial <G, W_orig> per tile  -> dot_part[w][tile]   (deterministic order)
//   2. every tile sums the partials of its weight and writes its share of the OIHW gradient
#define WGT_ROWS 64                                      // LDS rows per tile (taps x channels of the chunk, wgt_tg)
// A weight's un-packing is cut into tiles of 32 packed couts x one channel chunk x a GROUP OF TAPS of ~32 LDS rows, one
// workgroup each: a trunk layer (64 x 64 x 9) is 36 tiles with one memory round trip per phase (it was 4 tiles walking 9
// dependent rounds each: 26-30 us for the 37 layers of the generator, latency-bound with 150 busy workgroups).
__host__ __device__ __forceinline__ int wgt_tg(const SisrWeightGradDesc& w) {      // taps per tile
    const int ck = w.layout == 1 ? 32 : w.CK, nci = ck < w.Cin ? ck : w.Cin, taps = w.KH * w.KW;
    const int tg = nci > 0 ? 32 / nci : 1;
    return tg < 1 ? 1 : (tg > taps ? taps : tg);
}
__host__ __device__ __forceinline__ int wgt_base_tiles(const SisrWeightGradDesc& w) {
    const int ck = w.layout == 1 ? 32 : w.CK;
    return ((w.Cout + 31) / 32) * ((w.Cin + ck - 1) / ck);
}
__host__ __device__ __forceinline__ int wgt_tiles(const SisrWeightGradDesc& w) {
    const int tg = wgt_tg(w);
    return wgt_base_tiles(w) * ((w.KH * w.KW + tg - 1) / tg);
}

// mode 0: returns this thread's share of <G, W_orig> over the tile; mode 1: writes the gradient
template <int MODE>
__device__ __forceinline__ float wgt_tile(const SisrWeightGradDesc& w, int tile, float* lds, float gw, float inv) {
    const int tid = threadIdx.x;
    const int n_cot = (w.Cout + 31) / 32, n_base = wgt_base_tiles(w);
    const int base = tile % n_base, tgi = tile / n_base;
    const int cot = base % n_cot, chunk = base / n_cot;
    const int ck = w.layout == 1 ? 32 : w.CK;
    const int ci0 = chunk * ck, nci = min(ck, w.Cin - ci0);
    const int taps = w.KH * w.KW, cols = w.Cin * taps, Cq = w.Cout >> 2;
    const int tgroup = wgt_tg(w);                                   // taps of this tile (rows = taps x channels <= WGT_ROWS)
    float part = 0.f;
    for (int t0 = tgi * tgroup; t0 < min(taps, (tgi + 1) * tgroup); t0 += tgroup) {
        const int nt = min(tgroup, taps - t0), rows = nt * nci;
        __syncthreads();
        // 4 independent 128-byte-coalesced loads in flight per thread before the LDS stores (the tile is otherwise
        // one memory latency per 8 rows)
        for (int idx0 = tid; idx0 < rows * 32; idx0 += 4 * SISR_BLOCK) {
            float val[4];
            int off[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int idx = idx0 + k * SISR_BLOCK;
                val[k] = 0.f; off[k] = -1;
                if (idx < rows * 32) {
                    const int row = idx >> 5, c = idx & 31;
                    const int tl = row / nci, cl = row - tl * nci, tap = t0 + tl;
                    const int cp = cot * 32 + c;
                    int64_t prow;
                    if (w.layout == 1) prow = (int64_t)(chunk * taps + tap) * 32 + cl;
                    else { const int r = tap / w.KW, sx = tap - r * w.KW; prow = (int64_t)(chunk * w.KH + r) * w.KROWP + sx * w.PS + cl; }
                    off[k] = row * 33 + c;
                    if (cp < w.CoutPad) val[k] = w.dwpk[prow * w.CoutPad + cp];
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (off[k] >= 0) lds[off[k]] = val[k];
        }
        __syncthreads();
        for (int idx0 = tid; idx0 < rows * 32; idx0 += 4 * SISR_BLOCK) {
            float g[4], wv[4];
            int64_t e[4];
            int co_[4], col_[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int idx = idx0 + k * SISR_BLOCK;
                e[k] = -1; g[k] = wv[k] = 0.f; co_[k] = col_[k] = 0;
                if (idx < rows * 32) {
                    const int c = idx / rows, q = idx - c * rows;        // q runs over (cl, tap): contiguous in OIHW
                    const int cl = q / nt, tl = q - cl * nt;
                    const int cp = cot * 32 + c;
                    if (cp < w.Cout) {
                        co_[k] = w.shuffle2 ? ((cp % Cq) * 4 + cp / Cq) : cp;
                        col_[k] = (ci0 + cl) * taps + t0 + tl;
                        e[k] = (int64_t)co_[k] * cols + col_[k];
                        g[k] = lds[(tl * nci + cl) * 33 + c];
                        if (MODE == 0) wv[k] = w.w_orig[e[k]];
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (e[k] < 0) continue;
                if (MODE == 0) part += g[k] * wv[k];
                else w.grad[e[k]] = w.u_used ? (g[k] - gw * w.u_used[co_[k]] * w.v_used[col_[k]]) * inv : g[k];
            }
        }
    }
    return part;
}

__global__ void __launch_bounds__(SISR_BLOCK) weights_grad_dot_kernel(const SisrWeightGradDesc* table, float* dot_part) {
    __shared__ float lds[WGT_ROWS * 33];
    __shared__ float scratch[8];
    const SisrWeightGradDesc w = table[blockIdx.x];
    if ((int)blockIdx.y >= wgt_tiles(w)) return;
    float part = 0.f;
    if (w.u_used != nullptr && w.grad != nullptr) part = wgt_tile<0>(w, blockIdx.y, lds, 0.f, 0.f);
    const float tot = block_sum(part, scratch);
    if (threadIdx.x == 0) dot_part[(int64_t)blockIdx.x * gridDim.y + blockIdx.y] = tot;
}

__global__ void __launch_bounds__(SISR_BLOCK) weights_grad_kernel(const SisrWeightGradDesc* table, const float* dot_part) {
    __shared__ float lds[WGT_ROWS * 33];
    __shared__ float scratch[8];
    const SisrWeightGradDesc w = table[blockIdx.x];
    const int tid = threadIdx.x, n_tiles = wgt_tiles(w);
    if ((int)blockIdx.y >= n_tiles) return;
    const int Cq = w.Cout >> 2;
    if (blockIdx.y == 0 && w.grad_bias != nullptr && w.dbias_pk != nullptr) {
        for (int co = tid; co < w.Cout; co += SISR_BLOCK)
            w.grad_bias[co] = w.dbias_pk[w.shuffle2 ? ((co & 3) * Cq + (co >> 2)) : co];
    }
    if (w.grad == nullptr) return;
    float gw = 0.f, inv = 1.f;
    if (w.u_used != nullptr) {
        const float sigma = w.sigma[0];
        // (a large layer has thousands of tiles: the partial dots are summed by the workgroup, fixed partition and order,
        // not by every thread on its own)
        float dot = 0.f;
        for (int k = tid; k < n_tiles; k += SISR_BLOCK) dot += dot_part[(int64_t)blockIdx.x * gridDim.y + k];
        dot = block_sum(dot, scratch);
        gw = dot / sigma;          // <G, W> with W = W_orig / sigma
        inv = 1.f / sigma;
    }
    wgt_tile<1>(w, blockIdx.y, lds, gw, inv);
}

// ---- fast path of the weight-gradient epilogue for the 3x3 layers of the bf16 build (slab layout 1, channels in 32s) -------------
// The generic pair above cuts a 512 x 512 x 3 x 3 weight into 2,304 tiles of 32 rows and reads it twice (dot, then gradient): 166 us
// per discriminator backward.  Here a workgroup takes a whole 32-cout x 32-cin x 9-tap tile (288 packed rows of 128 bytes in,
// 32 OIHW rows of 1,152 contiguous bytes out) through LDS ONCE: it writes grad = G / sigma and its share of <G, W_orig>; the
// rank-one spectral-norm term -<G, W> u v^T / sigma is an elementwise pass over the finished OIHW gradient afterwards.
__global__ void __launch_bounds__(SISR_BLOCK) weights_grad_fast_kernel(const SisrWeightGradDesc* table, float* dot_part) {
    __shared__ float tile[288][33];
    __shared__ float scratch[8];
    const SisrWeightGradDesc w = table[blockIdx.x];
    const int cb = blockIdx.y, kb = blockIdx.z, tid = threadIdx.x;
    const int ncb = (w.Cout + 31) >> 5, nkb = w.Cin >> 5;
    if (cb >= ncb || kb >= nkb) return;
    if (cb == 0 && kb == 0 && w.grad_bias != nullptr && w.dbias_pk != nullptr)
        for (int co = tid; co < w.Cout; co += SISR_BLOCK) w.grad_bias[co] = w.dbias_pk[co];
    float part = 0.f;
    if (w.grad != nullptr) {
        const float inv = w.u_used != nullptr ? 1.f / w.sigma[0] : 1.f;
        // packed rows (tap, ci) of chunk kb: dwpk[((kb * 9 + tap) * 32 + ci) * CoutPad + cb * 32 + c]; CoutPad % 32 == 0 here
        // (the caller's dispatch rule), so a row's 32 couts are eight aligned float4s
        const float* src = w.dwpk + (int64_t)kb * 288 * w.CoutPad + cb * 32;
        const bool full = cb * 32 + 32 <= w.CoutPad;
        for (int i = tid; i < 288 * 8; i += SISR_BLOCK) {
            const int row = i >> 3, c4 = i & 7;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (full) v = *reinterpret_cast<const f32x4*>(src + (int64_t)row * w.CoutPad + c4 * 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) tile[row][c4 * 4 + j] = v[j];
        }
        __syncthreads();
        // OIHW rows: grad[co][kb * 32 + ci][tap], 288 contiguous floats per cout (1,152-byte rows); element e = ci * 9 + tap
        // <- tile[tap * 32 + ci][co]; one float4 of the row per item
        for (int i = tid; i < 32 * 72; i += SISR_BLOCK) {
            const int co = i / 72, e4 = i - co * 72;
            if (cb * 32 + co >= w.Cout) continue;
            const int64_t o = ((int64_t)(cb * 32 + co) * w.Cin + kb * 32) * 9 + e4 * 4;
            f32x4 g;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int e = e4 * 4 + j, ci = e / 9, tap = e - ci * 9;
                g[j] = tile[tap * 32 + ci][co];
            }
            if (w.u_used != nullptr) {
                const f32x4 wo = *reinterpret_cast<const f32x4*>(w.w_orig + o);
                part += (g[0] * wo[0] + g[1] * wo[1]) + (g[2] * wo[2] + g[3] * wo[3]);
            }
            *reinterpret_cast<f32x4*>(w.grad + o) = g * inv;
        }
    }
    const float tot = block_sum(part, scratch);
    if (tid == 0) dot_part[((int64_t)blockIdx.x * gridDim.y + cb) * gridDim.z + kb] = tot;
}

// grad[co][j] -= (<G, W_orig> / sigma^2) u[co] v[j]      (W = W_orig / sigma; dW_orig = (G - <G, W> u v^T) / sigma)
__global__ void __launch_bounds__(SISR_BLOCK) weights_grad_rank1_kernel(const SisrWeightGradDesc* table, const float* dot_part,
                                                                        int tiles_y, int tiles_z) {
    __shared__ float scratch[8];
    const SisrWeightGradDesc w = table[blockIdx.x];
    if (w.u_used == nullptr || w.grad == nullptr) return;
    const int ncb = (w.Cout + 31) >> 5, nkb = w.Cin >> 5, tid = threadIdx.x;
    float dot = 0.f;
    for (int k = tid; k < ncb * nkb; k += SISR_BLOCK) dot += dot_part[((int64_t)blockIdx.x * tiles_y + k / nkb) * tiles_z + k % nkb];
    dot = block_sum(dot, scratch);                                      // fixed partition and order: every workgroup gets the same bits
    const float sigma = w.sigma[0];
    const float coef = dot / (sigma * sigma);
    const int cols = w.Cin * 9;
    const int64_t total = (int64_t)w.Cout * cols;
    for (int64_t e = (int64_t)blockIdx.y * SISR_BLOCK + tid; e < total; e += (int64_t)gridDim.y * SISR_BLOCK) {
        const int co = (int)(e / cols), j = (int)(e - (int64_t)co * cols);
        w.grad[e] -= coef * w.u_used[co] * w.v_used[j];
    }
}

static int parts_for(int64_t elems) {           // workgroups per weight for the element-wise multi-tensor kernels
    const int64_t want = (elems + 4095) / 4096;   // ~16 elements per thread
    return (int)std::max<int64_t>(16, std::min<int64_t>(want, 1024));
}

// the three parts of sisr_weights_prepare as entry points of their own: a caller that keeps packed images across forwards
// (W_orig does not change between two optimizer steps; only u, v, sigma do) runs the power iteration alone
extern "C" int sisr_weights_sn(const SisrWeightDesc* table_dev, int32_t n, int32_t max_rows, int32_t max_cols, void* stream) {
    if (!table_dev || n <= 0 || max_rows <= 0 || max_cols <= 0) return SISR_E_BADARG;
    hipStream_t st = sisr_stream(stream);
    const int jobs_a = ((max_rows + SN_RB - 1) / SN_RB) * ((max_cols + SN_CB - 1) / SN_CB);
    hipLaunchKernelGGL(sn_wt_u_kernel, dim3(n, jobs_a), dim3(SISR_BLOCK), 0, st, table_dev);
    SISR_CHECK_LAUNCH();
    hipLaunchKernelGGL(sn_t_sum_kernel, dim3(n, (max_cols + SISR_BLOCK - 1) / SISR_BLOCK), dim3(SISR_BLOCK), 0, st, table_dev);
    SISR_CHECK_LAUNCH();
    hipLaunchKernelGGL(sn_w_v_kernel, dim3(n, (max_rows + 3) / 4), dim3(SISR_BLOCK), 0, st, table_dev);
    SISR_CHECK_LAUNCH();
    hipLaunchKernelGGL(sn_u_finish_kernel, dim3(n), dim3(SISR_BLOCK), 0, st, table_dev);
    SISR_CHECK_LAUNCH();
    return 0;
}

extern "C" int sisr_weights_pack(const SisrWeightDesc* table_dev, int32_t n, int32_t max_rows, int32_t max_cols, void* stream) {
    if (!table_dev || n <= 0 || max_rows <= 0 || max_cols <= 0) return SISR_E_BADARG;
    hipStream_t st = sisr_stream(stream);
    // packed images are a little larger than the matrix (padding slots): parts from 2x its size
    hipLaunchKernelGGL(weights_pack_kernel, dim3(n, parts_for(2ll * max_rows * max_cols)), dim3(SISR_BLOCK), 0, st, table_dev);
    SISR_CHECK_LAUNCH();
    return 0;
}

// the conv_deep.hip images (wdp_*) of every 3x3 weight of the table that asks for one; max_cout / max_cin over those weights
extern "C" int sisr_weights_pack_deep(const SisrWeightDesc* table_dev, int32_t n, int32_t max_cout, int32_t max_cin, void* stream) {
    if (!table_dev || n <= 0 || max_cout <= 0 || max_cin <= 0) return SISR_E_BADARG;
    hipStream_t st = sisr_stream(stream);
    hipLaunchKernelGGL(weights_pack_deep_kernel, dim3(n, (max_cout + 31) / 32, (max_cin + 31) / 32), dim3(SISR_BLOCK), 0, st, table_dev);
    SISR_CHECK_LAUNCH();
    return 0;
}

extern "C" int sisr_weights_prepare(const SisrWeightDesc* table_dev, int32_t n, int32_t max_rows, int32_t max_cols,
                                    void* stream) {
    if (int e = sisr_weights_sn(table_dev, n, max_rows, max_cols, stream)) return e;
    return sisr_weights_pack(table_dev, n, max_rows, max_cols, stream);
}

extern "C" int64_t sisr_weight_image_bytes(const SisrWeightImage* g) {
    if (!g || g->format < SISR_WIMG_F32 || g->format > SISR_WIMG_DEEP || g->KH <= 0 || g->KW <= 0 || g->n_chunk <= 0 || g->CoutPad <= 0 ||
        g->extra < 0 || (g->format == SISR_WIMG_F32 ? g->KROWP <= 0 || g->PS <= 0 || g->CK <= 0 || g->extra > 2
                         : g->format == SISR_WIMG_BF16 ? g->CK <= 0 || g->extra > 1 : g->extra < g->KW))
        return SISR_E_BADARG;
    return wimg_bytes(*g);
}

// tiles (= workgroups along grid.y, = dot_work entries) one weight of the table needs; `parts` of sisr_weights_grad must
// be >= the maximum over the table
extern "C" int sisr_weights_grad_tiles(const SisrWeightGradDesc* w) {
    if (!w || w->Cout <= 0 || w->Cin <= 0 || w->KH <= 0 || w->KW <= 0 || (w->layout != 1 && w->CK <= 0)) return SISR_E_BADARG;
    return wgt_tiles(*w);
}

// every weight of the table: 3x3, Cin % 32 == 0, layout 1 (bf16-kernel slabs), no PixelShuffle permutation.
// dot_work: n * ceil(max_cout / 32) * (max_cin / 32) floats.
extern "C" int sisr_weights_grad_fast(const SisrWeightGradDesc* table_dev, int32_t n, float* dot_work, int32_t max_cout,
                                      int32_t max_cin, void* stream) {
    if (!table_dev || n <= 0 || !dot_work || max_cout <= 0 || max_cin < 32) return SISR_E_BADARG;
    hipStream_t st = sisr_stream(stream);
    const int ty = (max_cout + 31) / 32, tz = max_cin / 32;
    hipLaunchKernelGGL(weights_grad_fast_kernel, dim3(n, ty, tz), dim3(SISR_BLOCK), 0, st, table_dev, dot_work);
    SISR_CHECK_LAUNCH();
    const int parts = (int)std::max<int64_t>(8, std::min<int64_t>(((int64_t)max_cout * max_cin * 9 + 4095) / 4096, 512));
    hipLaunchKernelGGL(weights_grad_rank1_kernel, dim3(n, parts), dim3(SISR_BLOCK), 0, st, table_dev, dot_work, ty, tz);
    SISR_CHECK_LAUNCH();
    return 0;
}

extern "C" int sisr_weights_grad(const SisrWeightGradDesc* table_dev, int32_t n, float* dot_work, int32_t parts,
                                 void* stream) {
    if (!table_dev || n <= 0 || !dot_work || parts <= 0 || parts > 65535) return SISR_E_BADARG;
    hipStream_t st = sisr_stream(stream);
    hipLaunchKernelGGL(weights_grad_dot_kernel, dim3(n, parts), dim3(SISR_BLOCK), 0, st, table_dev, dot_work);
    SISR_CHECK_LAUNCH();
    hipLaunchKernelGGL(weights_grad_kernel, dim3(n, parts), dim3(SISR_BLOCK), 0, st, table_dev, dot_work);
    SISR_CHECK_LAUNCH();
    return 0;
}
