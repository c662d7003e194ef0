// conv_bf16.hip -- direct convolution on gfx950 with bf16 matrix cores (v_mfma_f32_32x32x16_bf16,
// fp32 accumulate).  Same workgroup/tile structure and the same fused prologues/epilogues as
// conv_fwd.hip; activations stay fp32 in HBM this round, they are converted to bf16 (RNE) while being
// staged into LDS, so the layer moves its algorithmic bytes once and the contraction runs at the
// bf16 MFMA rate (16x the exact-fp32 rate) -- which makes it HBM-bound, the regime BASELINE.json's
// north_star asks for.  Channel chunks of 32; requirements: Cin % 32 == 0, KH*KW <= 9.
//
// LDS images (bf16):
//   input  [pixel][PS = 40]   80-byte pixel stride: the 16-byte A fragments (8 consecutive channels
//          of one pixel) of 16 consecutive pixels fall on 16 distinct 16-byte slots (conflict-free
//          ds_read_b128); slots 32..39 are never read.
//   weight [cout][WS = taps*32 + 8]   592-byte rows (= 16 * odd): B fragments conflict-free too.
// MFMA 32x32x16 operand maps (cdna_hip_programming.md section 3): lane l holds A[row = l&31][k = 8*(l>>5)+j],
// B[k = 8*(l>>5)+j][col = l&31], j = 0..7; C/D as for the fp32 32x32 form.
#include "sisr_dev.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "sisr_bf16_stage.h"
#include "sisr_instr.h"

// Phase timeline of the generic kernel (developer build only: `make trace` -> libsisr_hip_trace.so, read by
// tools/trace_conv.py).  Thread 0 of each workgroup of the grid's z = 0 plane (the other planes have no slots) stamps the
// 100 MHz wall clock at phase boundaries.  (The z test sits in `end` -- no slots outside that plane -- and not in `who`: written
// there the compiler orders the tests differently and the trace build's device code changes.)
SISR_TRACE_BUFFER(sisr_trace, 4096, 16)
#define TR(k) SISR_TRACE_STAMP_ROW(sisr_trace, threadIdx.x == 0, blockIdx.y * gridDim.x + blockIdx.x, k, blockIdx.z == 0 ? 16 : 0, wall_clock64())

// merge two (count, mean, M2) partials (Chan, Golub, LeVeque); either side may be empty
__device__ __forceinline__ void stat_merge(float& n, float& mu, float& m2, float nb, float mub, float m2b) {
    const float nt = n + nb;
    if (nt > 0.f) {
        const float dl = mub - mu, f = nb / nt;
        mu += dl * f;
        m2 += m2b + dl * dl * n * f;
    }
    n = nt;
}

__device__ __forceinline__ f32x16 mfma_bf16(bf16x8 a, bf16x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

// one filter tap (32 input channels = two K=16 steps): all LDS fragment reads, then the MFMAs
template <int MSUB, int NSUB>
__device__ __forceinline__ void conv_bf16_tap(const __bf16* const (&ap)[MSUB], const __bf16* const (&bp)[NSUB],
                                              int aoff, int boff, f32x16 (&acc)[MSUB][NSUB]) {
    bf16x8 a[2][MSUB], b[2][NSUB];
#pragma unroll
    for (int kc = 0; kc < 2; ++kc) {
#pragma unroll
        for (int ms = 0; ms < MSUB; ++ms) a[kc][ms] = *reinterpret_cast<const bf16x8*>(ap[ms] + aoff + kc * 16);
#pragma unroll
        for (int ns = 0; ns < NSUB; ++ns) b[kc][ns] = *reinterpret_cast<const bf16x8*>(bp[ns] + boff + kc * 16);
    }
#pragma unroll
    for (int kc = 0; kc < 2; ++kc)
#pragma unroll
        for (int ms = 0; ms < MSUB; ++ms)
#pragma unroll
            for (int ns = 0; ns < NSUB; ++ns) acc[ms][ns] = mfma_bf16(a[kc][ms], b[kc][ns], acc[ms][ns]);
    __builtin_amdgcn_sched_group_barrier(0x100, 2 * (MSUB + NSUB), 0);
    __builtin_amdgcn_sched_group_barrier(0x008, 2 * MSUB * NSUB, 0);
}

// XBF / YBF: storage type of the input operand (x1, x2) and of the output side (y, res, bnb_x): compile-time so that
// each instantiation carries one staging family and one epilogue (registers: 3 waves per SIMD for the 128-pixel tiles)
template <int MSUB, int NSUB, int TAG, bool XBF, bool YBF>
__global__ void __launch_bounds__(SISR_BLOCK, 2) conv_mfma_bf16_kernel(const SisrConvDesc d) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const SisrConvPlan& p = d.plan;
    constexpr int BM = 4 * MSUB * 32, BN = NSUB * 32;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, kk = lane >> 5;
    const int S = d.stride;
    const int IH = (p.TH - 1) * S + d.KH, IW = (p.TW - 1) * S + d.KW;
    const int npix = p.TN * IH * IW;
    const int taps = d.KH * d.KW;
    const int WSG = taps * BF_CK, WS = WSG + 8;

    int* row_off = reinterpret_cast<int*>(smem);
    __bf16* lds_in = reinterpret_cast<__bf16*>(smem + BM);
    __bf16* lds_w = lds_in + ((npix * BF_PS + 16 + 7) & ~7);
    float* red = reinterpret_cast<float*>(lds_w);            // epilogue scratch (12*BN floats)

    TR(0);
#ifdef SISR_CONV_TRACE
    if (tid == 0 && blockIdx.y * gridDim.x + blockIdx.x < sisr_trace_wgs && blockIdx.z == 0) {
        unsigned hwid;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
        unsigned xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        sisr_trace_buf[(blockIdx.y * gridDim.x + blockIdx.x) * sisr_trace_slots + 15] = ((unsigned long long)xcc << 32) | hwid;
    }
#endif
    // packed weights [chunk][CoutPad][WSG] bf16: a workgroup's slice of one chunk is contiguous, 16-byte vector
    // v of it goes to LDS row v / wvec_row.  WVEC vectors per thread cover BN * WSG <= 64 * 288 elements.
    constexpr int WVEC = (BN * 9 * BF_CK / 8 + SISR_BLOCK - 1) / SISR_BLOCK;
    const int wvec_row = WSG >> 3;                       // 16-byte vectors per packed weight row
    const int wvecs = BN * wvec_row;
    const __amdgpu_buffer_rsrc_t wrs = bf_rsrc(d.wpk, (unsigned)p.wpk_elems * 2u);
    // no per-lane predicate on the loads: vectors past the slice are in-bounds of the buffer (or read as zeros
    // past its end) and are simply not written to LDS
    const unsigned wvoff = (unsigned)tid * 16u;
    bf16x8 wv[WVEC];
    {
        const unsigned cb = (unsigned)((blockIdx.z * BN) * WSG) * 2u;
#pragma unroll
        for (int u = 0; u < WVEC; ++u)
            if (u * SISR_BLOCK < wvecs)
                wv[u] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(wrs, wvoff + u * (SISR_BLOCK * 16), cb, 0));
    }
    // grid = (tiles of one image group, image groups, cout tiles); index arithmetic by reciprocal multiplies
    const int tyi = fdiv(blockIdx.x, p.m_tiles_x), txi = blockIdx.x - tyi * p.tiles_x, ng = blockIdx.y;
    const int tile_id = blockIdx.y * gridDim.x + blockIdx.x;
    const int n0 = ng * p.TN, oy0 = tyi * p.TH, ox0 = txi * p.TW;
    const int cout_base = blockIdx.z * BN;
    const int thw = p.TH * p.TW, tile_rows = p.TN * thw;

    for (int m = tid; m < BM; m += SISR_BLOCK) {
        int off = -1;
        if (m < tile_rows) {
            const int tn = fdiv(m, p.m_thw), rem = m - tn * thw;
            const int ty = fdiv(rem, p.m_tw), tx = rem - ty * p.TW;
            const int n = n0 + tn, oy = oy0 + ty, ox = ox0 + tx;
            if (n < d.N && oy < d.Ho && ox < d.Wo) {
                const int py = oy * d.y_sy + d.y_oy, px = ox * d.y_sx + d.y_ox;
                if (d.y_mode == SISR_Y_NHWC)
                    off = ((n * d.y_H + py) * d.y_W + px) * d.Cout;
                else if (d.y_mode == SISR_Y_NCHW)
                    off = n * d.Cout * d.y_H * d.y_W + py * d.y_W + px;
                else
                    off = ((n * 2 * d.Ho + 2 * oy) * (2 * d.Wo) + 2 * ox) * (d.Cout >> 2);
            }
        }
        row_off[m] = off;
    }

    TR(13);
    const __bf16* ap[MSUB];
    const __bf16* bp[NSUB];
#pragma unroll
    for (int ms = 0; ms < MSUB; ++ms) {
        const int m = wave * (MSUB * 32) + ms * 32 + l31;
        int base = 0;
        if (m < tile_rows) {
            const int tn = fdiv(m, p.m_thw), rem = m - tn * thw;
            const int ty = fdiv(rem, p.m_tw), tx = rem - ty * p.TW;
            base = ((tn * IH + ty * S) * IW + tx * S) * BF_PS;
        }
        ap[ms] = lds_in + base + 8 * kk;
    }
#pragma unroll
    for (int ns = 0; ns < NSUB; ++ns) bp[ns] = lds_w + (ns * 32 + l31) * WS + 8 * kk;

    f32x16 acc[MSUB][NSUB];
#pragma unroll
    for (int ms = 0; ms < MSUB; ++ms)
#pragma unroll
        for (int ns = 0; ns < NSUB; ++ns)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[ms][ns][i] = 0.f;

    TR(14);
    OperandView ov;
    ov.x1 = d.x1; ov.x2 = d.x2; ov.pa = d.pa; ov.pb = d.pb; ov.pd = d.pd; ov.ps = d.ps; ov.pt = d.pt;
    ov.N = d.N; ov.H = d.H; ov.W = d.W; ov.C = d.Cin;
    ov.mode = d.x_mode; ov.pro = d.pro_mode;
    ov.slope = d.pro_slope_p ? d.pro_slope_p[0] : d.pro_slope;
    ov.bf16 = d.x_bf16;
    const int iy_org = oy0 * S - d.pad_y, ix_org = ox0 * S - d.pad_x;
    const int wstep_j = fdiv(SISR_BLOCK, p.m_wrow), wstep_k = SISR_BLOCK - wstep_j * wvec_row;
    const int wstep_off = wstep_j * WS + wstep_k * 8;
    const int wj0 = fdiv(tid, p.m_wrow), wk0 = tid - wj0 * wvec_row, woff0 = wj0 * WS + wk0 * 8;

    for (int chunk = 0; chunk < p.n_chunk; ++chunk) {
        __syncthreads();   // all fragment reads of the previous chunk are done
        TR(1 + 4 * (chunk & 1));
        stage_operand_tile_bf16<8, XBF ? 1 : 0>(ov, lds_in, BF_PS, BF_CK, chunk * BF_CK, p.TN, IH, IW, n0, iy_org, ix_org, 1 << 30, p.m_iw);
        TR(2 + 4 * (chunk & 1));
        {   // this chunk's packed weights are already in registers (loaded during the previous MFMA phase / the
            // kernel prologue): write them to LDS, then put the next chunk's loads in flight
            int wk = wk0, woff = woff0;
#pragma unroll
            for (int u = 0; u < WVEC; ++u) {
                if (tid + u * SISR_BLOCK < wvecs) *reinterpret_cast<bf16x8*>(lds_w + woff) = wv[u];
                wk += wstep_k; woff += wstep_off;
                if (wk >= wvec_row) { wk -= wvec_row; woff += 8; }
            }
            if (chunk + 1 < p.n_chunk) {
                const unsigned cb = (unsigned)(((chunk + 1) * p.CoutPad + cout_base) * WSG) * 2u;
#pragma unroll
                for (int u = 0; u < WVEC; ++u)
                    if (u * SISR_BLOCK < wvecs)
                        wv[u] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(wrs, wvoff + u * (SISR_BLOCK * 16), cb, 0));
            }
        }
        TR(3 + 4 * (chunk & 1));
        __syncthreads();
        TR(4 + 4 * (chunk & 1));
        int tap = 0;
        for (int r = 0; r < d.KH; ++r)
            for (int s = 0; s < d.KW; ++s, ++tap)
                conv_bf16_tap<MSUB, NSUB>(ap, bp, (r * IW + s) * BF_PS, tap * BF_CK, acc);
    }
    TR(9);
    __syncthreads();   // LDS (weights region) is reused as reduction scratch below
    TR(10);

    // ---- epilogue (identical to conv_fwd.hip: the 32x32 accumulator layout is dtype independent) ----
    int col_off[NSUB];
    bool col_ok[NSUB];
#pragma unroll
    for (int ns = 0; ns < NSUB; ++ns) {
        const int cp = cout_base + ns * 32 + l31;
        col_ok[ns] = cp < d.Cout;
        int co = cp;
        col_off[ns] = cp;
        if (d.y_mode == SISR_Y_NHWC_SHUFFLE2) {
            const int Cq = d.Cout >> 2;
            const int ij = cp / Cq, c = cp - ij * Cq;
            co = c * 4 + ij;
            col_off[ns] = ((ij >> 1) * (2 * d.Wo) + (ij & 1)) * Cq + c;
        } else if (d.y_mode == SISR_Y_NCHW) {
            col_off[ns] = cp * d.y_H * d.y_W;
        }
        const float bv = (d.bias != nullptr && col_ok[ns]) ? d.bias[co] : 0.f;
#pragma unroll
        for (int ms = 0; ms < MSUB; ++ms)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[ms][ns][i] += bv;
    }

    // this lane's accumulator rows: byte offset of the output pixel, or the out-of-range marker 2^31 (tensors
    // are < 2 GB, so marker + any channel offset stays out of range and the hardware drops the access)
    unsigned rb[MSUB][16];
    bool rv[MSUB][16];
#pragma unroll
    for (int ms = 0; ms < MSUB; ++ms)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int o = row_off[wave * (MSUB * 32) + ms * 32 + mfma_row(i, lane)];
            rv[ms][i] = o >= 0;
            rb[ms][i] = o >= 0 ? (unsigned)o * 4u : 0x80000000u;
        }

    if (d.stat_part != nullptr) {
        // BatchNorm statistics of the tile, one pass: every lane reduces its rows to (count, mean, M2), the
        // partials are merged pairwise (Chan et al.) -- lane halves by a shuffle, the 4 waves through LDS in a
        // fixed order (deterministic) -- one barrier instead of a two-pass mean / deviation scheme
        float n = 0.f;
#pragma unroll
        for (int ms = 0; ms < MSUB; ++ms)
#pragma unroll
            for (int i = 0; i < 16; ++i) n += rv[ms][i] ? 1.f : 0.f;
        const float inv = n > 0.f ? 1.f / n : 0.f;
        const float n_o = __shfl_xor(n, 32);
#pragma unroll
        for (int ns = 0; ns < NSUB; ++ns) {
            float sm = 0.f;
#pragma unroll
            for (int ms = 0; ms < MSUB; ++ms)
#pragma unroll
                for (int i = 0; i < 16; ++i) sm += rv[ms][i] ? acc[ms][ns][i] : 0.f;
            float mu = sm * inv, m2 = 0.f;
#pragma unroll
            for (int ms = 0; ms < MSUB; ++ms)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const float dv = acc[ms][ns][i] - mu;
                    m2 += rv[ms][i] ? dv * dv : 0.f;
                }
            float nn = n;
            stat_merge(nn, mu, m2, n_o, __shfl_xor(mu, 32), __shfl_xor(m2, 32));
            if (kk == 0) {
                float* r = red + (wave * BN + ns * 32 + l31) * 3;
                r[0] = nn; r[1] = mu; r[2] = m2;
            }
        }
        __syncthreads();
        if (tid < BN && cout_base + tid < d.Cout) {
            float nn = red[tid * 3], mu = red[tid * 3 + 1], m2 = red[tid * 3 + 2];
#pragma unroll
            for (int w = 1; w < 4; ++w) {
                const float* r = red + (w * BN + tid) * 3;
                stat_merge(nn, mu, m2, r[0], r[1], r[2]);
            }
            float* sp = d.stat_part + (int64_t)tile_id * 2 * d.Cout + cout_base + tid;
            sp[0] = mu;
            sp[d.Cout] = m2;
            if (tid == 0 && blockIdx.z == 0) d.cnt_part[tile_id] = nn;
        }
    }
    TR(11);

    const unsigned ypix = (unsigned)max(d.N * d.y_H * d.y_W, d.N * d.Ho * d.Wo);
    if constexpr (YBF) {
        // ---- bf16 tensors in HBM (NHWC / pixel-shuffled NHWC output): every global access of the epilogue is a
        // 16-byte access of 8 consecutive channels of one pixel; the change between that layout and the accumulator
        // layout (lane = channel, registers = pixels) goes through LDS with the transposing read ds_read_b64_tr_b16:
        //   residual / BatchNorm input: global -> [pixel][RS] image -> transposed read = 4 consecutive pixels of the
        //   lane's channel = one accumulator register group;  output: 4 pixels of a register group packed (8 bytes)
        //   -> [channel][YS] image -> transposed read = 4 consecutive channels of one pixel, two reads = 16 bytes.
        constexpr int RS = BN + 8, YS = BM + 4, OCT = BN / 8;
        __bf16* img_r = lds_in;
        __bf16* img_x = lds_in + BM * RS;
        __bf16* img_y = reinterpret_cast<__bf16*>(red + 12 * BN);
        const unsigned ybytes2 = ypix * (unsigned)d.Cout * 2u;
        const int grp = lane >> 4, tq = (lane & 15) >> 2, tp = lane & 3;
        const bool has_r = d.res != nullptr, has_x = d.bnb_part != nullptr;
        s16x4 pr[MSUB][NSUB][4], px[MSUB][NSUB][4];
        if (has_r || has_x) {
            const __amdgpu_buffer_rsrc_t rr = bf_rsrc(has_r ? d.res : d.bnb_x, ybytes2);
            const __amdgpu_buffer_rsrc_t rx = bf_rsrc(has_x ? d.bnb_x : d.res, ybytes2);
            constexpr int ITEMS = BM * OCT / SISR_BLOCK;           // 16-byte items per thread and tensor
            u32x4 vr[ITEMS], vx[ITEMS];
#pragma unroll
            for (int k = 0; k < ITEMS; ++k) {
                const int idx = tid + k * SISR_BLOCK, m = idx / OCT, oc = idx - m * OCT;
                const int ro = row_off[m], ch = cout_base + oc * 8;
                const unsigned vo = (ro >= 0 && ch < d.Cout) ? (unsigned)(ro + ch) * 2u : 0x80000000u;
                if (has_r) vr[k] = __builtin_amdgcn_raw_buffer_load_b128(rr, vo, 0, 0);
                if (has_x) vx[k] = __builtin_amdgcn_raw_buffer_load_b128(rx, vo, 0, 0);
            }
#pragma unroll
            for (int k = 0; k < ITEMS; ++k) {
                const int idx = tid + k * SISR_BLOCK, m = idx / OCT, oc = idx - m * OCT;
                if (has_r) *reinterpret_cast<u32x4*>(img_r + m * RS + oc * 8) = vr[k];
                if (has_x) *reinterpret_cast<u32x4*>(img_x + m * RS + oc * 8) = vx[k];
            }
            __syncthreads();
#pragma unroll
            for (int ms = 0; ms < MSUB; ++ms)
#pragma unroll
                for (int ns = 0; ns < NSUB; ++ns)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        // this 16-lane group's block: pixels 8g + 4kk .. +3 (rows), channels 16 * (l31 >> 4) .. +15
                        const int off = (wave * (MSUB * 32) + ms * 32 + 8 * g + 4 * (grp >> 1) + tq) * RS + ns * 32 + 16 * (grp & 1) + 4 * tp;
                        if (has_r) pr[ms][ns][g] = lds_tr16(img_r + off);
                        if (has_x) px[ms][ns][g] = lds_tr16(img_x + off);
                    }
        }
        if (has_r) {
#pragma unroll
            for (int ms = 0; ms < MSUB; ++ms)
#pragma unroll
                for (int ns = 0; ns < NSUB; ++ns)
#pragma unroll
                    for (int i = 0; i < 16; ++i)
                        acc[ms][ns][i] += bf16_bits_to_f32((unsigned short)pr[ms][ns][i >> 2][i & 3]);
        }
        if (has_x) {
            // BatchNorm-backward reductions of the gradient tile just formed (see the fp32-storage branch below)
            const float bslope = d.bnb_slope_p ? d.bnb_slope_p[0] : d.bnb_slope;
            float ssl = 0.f;
            __syncthreads();                               // the images are consumed; `red` is free
#pragma unroll
            for (int ns = 0; ns < NSUB; ++ns) {
                const int cp = cout_base + ns * 32 + l31;
                float sc = 0.f, sf = 0.f, mu = 0.f, is = 0.f;
                if (col_ok[ns]) { sc = d.bnb_scale[cp]; sf = d.bnb_shift[cp]; mu = d.bnb_mean[cp]; is = d.bnb_invstd[cp]; }
                float s1 = 0.f, s2 = 0.f;
#pragma unroll
                for (int ms = 0; ms < MSUB; ++ms)
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const float xv = bf16_bits_to_f32((unsigned short)px[ms][ns][i >> 2][i & 3]);
                        float g = rv[ms][i] ? (float)acc[ms][ns][i] : 0.f;
                        if (d.bnb_act) {
                            const float z = sc * xv + sf;
                            if (!(z > 0.f)) { ssl += g * z; g *= bslope; }
                        }
                        s1 += g;
                        s2 += g * ((xv - mu) * is);
                    }
                s1 += __shfl_xor(s1, 32);
                s2 += __shfl_xor(s2, 32);
                if (kk == 0) { red[(wave * BN + ns * 32 + l31) * 2] = s1; red[(wave * BN + ns * 32 + l31) * 2 + 1] = s2; }
            }
            ssl = wave_sum(ssl);
            if (lane == 0) red[8 * BN + wave] = ssl;
            __syncthreads();
            float* wk = d.bnb_part + (int64_t)tile_id * (2 * d.Cout + 1);
            if (tid < BN && cout_base + tid < d.Cout) {
                float s1 = 0.f, s2 = 0.f;
#pragma unroll
                for (int w = 0; w < 4; ++w) { s1 += red[(w * BN + tid) * 2]; s2 += red[(w * BN + tid) * 2 + 1]; }
                wk[cout_base + tid] = s1;
                wk[d.Cout + cout_base + tid] = s2;
            }
            if (tid == 0 && blockIdx.z == 0) wk[2 * d.Cout] = red[8 * BN] + red[8 * BN + 1] + red[8 * BN + 2] + red[8 * BN + 3];
        } else if (has_r) {
            __syncthreads();                               // img_y may overlap the residual image
        }
        // output: accumulators -> bf16 -> [channel][YS] image (this wave's pixel columns only: no barrier needed)
#pragma unroll
        for (int ms = 0; ms < MSUB; ++ms)
#pragma unroll
            for (int ns = 0; ns < NSUB; ++ns)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    bf16x4 h;
#pragma unroll
                    for (int j = 0; j < 4; ++j) { const float v = acc[ms][ns][4 * g + j]; h[j] = (__bf16)v; }
                    *reinterpret_cast<bf16x4*>(img_y + (ns * 32 + l31) * YS + wave * (MSUB * 32) + ms * 32 + 8 * g + 4 * kk) = h;
                }
        const __amdgpu_buffer_rsrc_t ry = bf_rsrc(d.y, ybytes2);
        const int Cq = d.Cout >> 2;
        // pass: the two 16-lane groups of a wave half take two 16-pixel blocks, the halves take two channel octets
#pragma unroll
        for (int ps = 0; ps < MSUB * OCT / 2; ++ps) {
            const int pb = 2 * (ps / (OCT / 2)) + (grp & 1);              // 16-pixel block of this wave's rows
            const int oc = 2 * (ps % (OCT / 2)) + (grp >> 1);              // channel octet
            const int m0 = wave * (MSUB * 32) + 16 * pb;
            const __bf16* src = img_y + (oc * 8 + tq) * YS + m0 + 4 * tp;
            const s16x4 lo = lds_tr16(src), hi = lds_tr16(src + 4 * YS);
            const int ro = row_off[m0 + (lane & 15)];
            const int cp = cout_base + oc * 8;
            int choff = cp;
            if (d.y_mode == SISR_Y_NHWC_SHUFFLE2) {
                const int ij = cp / Cq, c = cp - ij * Cq;
                choff = ((ij >> 1) * (2 * d.Wo) + (ij & 1)) * Cq + c;
            }
            const unsigned vo = (ro >= 0 && cp < d.Cout) ? (unsigned)(ro + choff) * 2u : 0x80000000u;
            const s16x8 v8 = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v8), ry, vo, 0, 0);
        }
        TR(12);
        return;
    } else {
    // output (and residual) through raw buffer accesses with 32-bit byte offsets
    const unsigned ybytes = ypix * (unsigned)d.Cout * 4u;
    const __amdgpu_buffer_rsrc_t ry = bf_rsrc(d.y, ybytes);
    // fused BatchNorm-backward reductions (below): that BatchNorm's input at this lane's pixels, requested before
    // the residual so both sets of loads share one memory latency
    float bx[MSUB][NSUB][16];
    if (d.bnb_part != nullptr) {
        const __amdgpu_buffer_rsrc_t rx = bf_rsrc(d.bnb_x, ybytes);
#pragma unroll
        for (int ns = 0; ns < NSUB; ++ns)
#pragma unroll
            for (int ms = 0; ms < MSUB; ++ms)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const unsigned vo = col_ok[ns] ? rb[ms][i] + (unsigned)col_off[ns] * 4u : 0x80000000u;
                    bx[ms][ns][i] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rx, vo, 0, 0));
                }
    }
    if (d.res != nullptr) {
        const __amdgpu_buffer_rsrc_t rr = bf_rsrc(d.res, ybytes);
#pragma unroll
        for (int ns = 0; ns < NSUB; ++ns)
            if (col_ok[ns]) {
#pragma unroll
                for (int ms = 0; ms < MSUB; ++ms)
#pragma unroll
                    for (int i = 0; i < 16; ++i)
                        acc[ms][ns][i] += __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rr, rb[ms][i] + (unsigned)col_off[ns] * 4u, 0, 0));
            }
    }
    if (d.bnb_part != nullptr) {
        // BatchNorm-backward reductions of the gradient tile just formed (y + residual), see SisrConvDesc.bnb_*:
        // per lane over its rows, lane halves by a shuffle, the 4 waves through LDS (fixed order)
        const float bslope = d.bnb_slope_p ? d.bnb_slope_p[0] : d.bnb_slope;
        float ssl = 0.f;
        __syncthreads();                                   // `red` may still hold the forward statistics
#pragma unroll
        for (int ns = 0; ns < NSUB; ++ns) {
            const int cp = cout_base + ns * 32 + l31;
            float sc = 0.f, sf = 0.f, mu = 0.f, is = 0.f;
            if (col_ok[ns]) { sc = d.bnb_scale[cp]; sf = d.bnb_shift[cp]; mu = d.bnb_mean[cp]; is = d.bnb_invstd[cp]; }
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int ms = 0; ms < MSUB; ++ms)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const float xv = bx[ms][ns][i];
                    float g = rv[ms][i] ? (float)acc[ms][ns][i] : 0.f;
                    if (d.bnb_act) {
                        const float z = sc * xv + sf;
                        if (!(z > 0.f)) { ssl += g * z; g *= bslope; }
                    }
                    s1 += g;
                    s2 += g * ((xv - mu) * is);
                }
            s1 += __shfl_xor(s1, 32);
            s2 += __shfl_xor(s2, 32);
            if (kk == 0) { red[(wave * BN + ns * 32 + l31) * 2] = s1; red[(wave * BN + ns * 32 + l31) * 2 + 1] = s2; }
        }
        ssl = wave_sum(ssl);
        if (lane == 0) red[8 * BN + wave] = ssl;
        __syncthreads();
        float* wk = d.bnb_part + (int64_t)tile_id * (2 * d.Cout + 1);
        if (tid < BN && cout_base + tid < d.Cout) {
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int w = 0; w < 4; ++w) { s1 += red[(w * BN + tid) * 2]; s2 += red[(w * BN + tid) * 2 + 1]; }
            wk[cout_base + tid] = s1;
            wk[d.Cout + cout_base + tid] = s2;
        }
        if (tid == 0 && blockIdx.z == 0) wk[2 * d.Cout] = red[8 * BN] + red[8 * BN + 1] + red[8 * BN + 2] + red[8 * BN + 3];
    }
    if (d.epi_act == SISR_EPI_TANH) {
#pragma unroll
        for (int ms = 0; ms < MSUB; ++ms)
#pragma unroll
            for (int ns = 0; ns < NSUB; ++ns)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[ms][ns][i] = tanhf(acc[ms][ns][i]);
    }
#pragma unroll
    for (int ns = 0; ns < NSUB; ++ns)
        if (col_ok[ns]) {
#pragma unroll
            for (int ms = 0; ms < MSUB; ++ms)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    // (a bit_cast applied directly to a vector element reads element 0 with this compiler)
                    const float val = acc[ms][ns][i];
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(val), ry, rb[ms][i] + (unsigned)col_off[ns] * 4u, 0, 0);
                }
        }
    TR(12);
    }
}

// ---- host ------------------------------------------------------------------------------------------
static inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

static int conv_bf16_lds_bytes(int BM, int TN, int TH, int TW, int S, int KH, int KW, int BN) {
    const int IH = (TH - 1) * S + KH, IW = (TW - 1) * S + KW;
    const int in_elems = (TN * IH * IW * BF_PS + 16 + 7) & ~7;
    // weights, later the epilogue's reduction scratch (12*BN floats) followed by the [BN][BM+4] bf16 output image
    const int w_bytes = std::max(BN * (KH * KW * BF_CK + 8) * 2, 12 * BN * 4 + BN * (BM + 4) * 2);
    // bf16 residual / BatchNorm-input images [BM][BN+8] x 2 start at the input tile
    const int img_bytes = 2 * BM * (BN + 8) * 2;
    return BM * 4 + std::max(in_elems * 2 + w_bytes, img_bytes) + 16;
}

extern "C" int sisr_conv2d_plan_bf16(SisrConvDesc* d) {
    if (!d || d->N <= 0 || d->Cin <= 0 || d->Cout <= 0 || d->KH <= 0 || d->KW <= 0) return SISR_E_BADARG;
    if ((d->Cin % BF_CK) || d->KH * d->KW > 9) return SISR_E_UNSUPPORTED;
    if (d->stride != 1 && d->stride != 2) return SISR_E_BADARG;
    if (d->x_mode == SISR_X_NCHW) return SISR_E_UNSUPPORTED;
    if (d->x_mode == SISR_X_NHWC_UNSHUFFLE2 && ((d->Cin >> 2) & 3)) return SISR_E_UNSUPPORTED;
    if (d->y_mode == SISR_Y_NHWC_SHUFFLE2 && (d->Cout & 3)) return SISR_E_BADARG;
    SisrConvPlan& p = d->plan;
    std::memset(&p, 0, sizeof(p));
    const int64_t ypix = std::max((int64_t)d->N * d->y_H * d->y_W, (int64_t)d->N * d->Ho * d->Wo);
    // 32-bit buffer addressing: input < 4 GB, output < 2 GB (its out-of-range marker is 2^31)
    if (ypix * d->Cout >= (1ll << 29) || (int64_t)d->N * d->H * d->W * d->Cin >= (1ll << 30)) return SISR_E_TOOBIG;
    p.nsub = d->Cout <= 32 ? 1 : 2;
    const int BN = p.nsub * 32;
    p.CoutPad = round_up(d->Cout, BN);
    p.CK = BF_CK; p.PS = BF_PS; p.KROWP = d->KH * d->KW * BF_CK;
    p.n_chunk = d->Cin / BF_CK;
    const int64_t out_pix = (int64_t)d->N * d->Ho * d->Wo;
    const int S = d->stride;
    SisrConvPlan cand[2];
    int cand_lds[2] = {0, 0};
    double cand_cost[2] = {1e30, 1e30};
    for (int mi = 0; mi < 2; ++mi) {
        const int msub = 2 - mi, BM = 4 * msub * 32;
        SisrConvPlan q = p;
        q.msub = msub;
        double best = -1.0;
        int best_lds = 0;
        for (int TW = 1; TW <= std::min(d->Wo, BM); ++TW) {
            const int TH = std::min(d->Ho, BM / TW);
            int TN = 1;
            if (TH == d->Ho && TW == d->Wo) TN = std::max(1, std::min(d->N, BM / (TH * TW)));
            const int lds = conv_bf16_lds_bytes(BM, TN, TH, TW, S, d->KH, d->KW, BN);
            if (lds > 80 * 1024) continue;
            const int ty = (d->Ho + TH - 1) / TH, tx = (d->Wo + TW - 1) / TW, ngr = (d->N + TN - 1) / TN;
            const double eff = (double)out_pix / ((double)ty * tx * ngr * BM);
            const double halo = (double)(TH * TW) * S * S / ((double)((TH - 1) * S + d->KH) * ((TW - 1) * S + d->KW));
            const double score = eff * (0.6 + 0.4 * halo);
            if (score > best + 1e-9) {
                best = score; best_lds = lds;
                q.TH = TH; q.TW = TW; q.TN = TN; q.tiles_y = ty; q.tiles_x = tx; q.n_groups = ngr;
            }
        }
        if (best < 0) continue;
        const int64_t blocks = (int64_t)q.tiles_y * q.tiles_x * q.n_groups * (p.CoutPad / BN);
        cand[mi] = q;
        cand_lds[mi] = best_lds;
        cand_cost[mi] = (double)((blocks + 511) / 512) * BM * (mi == 0 ? 1.0 : 1.05);
    }
    const int pick = cand_cost[1] < cand_cost[0] ? 1 : 0;
    if (cand_cost[pick] > 1e29) return SISR_E_TOOBIG;
    p = cand[pick];
    p.n_tiles = p.tiles_y * p.tiles_x * p.n_groups;
    if (p.tiles_y * p.tiles_x >= 65536 || p.n_groups >= 65536) return SISR_E_TOOBIG;   // grid (x, y) and reciprocal range
    {
        const int IW = (p.TW - 1) * S + d->KW;
        p.m_tiles_x = fdiv_magic(p.tiles_x); p.m_thw = fdiv_magic(p.TH * p.TW); p.m_tw = fdiv_magic(p.TW);
        p.m_iw = fdiv_magic(IW); p.m_wrow = fdiv_magic(d->KH * d->KW * BF_CK / 8);
    }
    p.lds_bytes = cand_lds[pick];
    p.wpk_elems = p.n_chunk * p.CoutPad * p.KROWP;       // bf16 elements
    return 0;
}

template <int MSUB, int NSUB, int TAG, bool XBF, bool YBF>
static int launch_conv_bf16_t(const SisrConvDesc* d, hipStream_t st) {
    const dim3 grid(d->plan.tiles_x * d->plan.tiles_y, d->plan.n_groups, d->plan.CoutPad / (NSUB * 32));
    return sisr_launch<conv_mfma_bf16_kernel<MSUB, NSUB, TAG, XBF, YBF>>(grid, dim3(SISR_BLOCK), d->plan.lds_bytes, SISR_LDS_BASE_DEFAULT, st, *d);
}

// storage combinations: all fp32 | bf16 in, bf16 out | bf16 in, fp32 out (NCHW images) | fp32 in, bf16 out (gradients
// that enter the bf16 tensors from an fp32 producer)
template <int MSUB, int NSUB, int TAG>
static int launch_conv_bf16(const SisrConvDesc* d, hipStream_t st) {
    if (d->x_bf16) return d->y_bf16 ? launch_conv_bf16_t<MSUB, NSUB, TAG, true, true>(d, st) : launch_conv_bf16_t<MSUB, NSUB, TAG, true, false>(d, st);
    return d->y_bf16 ? launch_conv_bf16_t<MSUB, NSUB, TAG, false, true>(d, st) : launch_conv_bf16_t<MSUB, NSUB, TAG, false, false>(d, st);
}

// the kernel family sisr_conv2d_bf16 hands `d` to (the only place that orders these families)
extern "C" int32_t sisr_conv2d_bf16_route(const SisrConvDesc* d) {
    if (!d) return SISR_E_BADARG;
    if (d->deep.enabled && d->wdeep) return SISR_ROUTE_DEEP;                    // planned for conv_deep.hip: runs there or is refused
    if (sisr_conv2d_toimage_eligible(d)) return SISR_ROUTE_TOIMAGE;             // the generator's last conv (64 -> 3)
    // the generator's trunk geometry: persistent weights-in-registers kernel
    return sisr_conv2d_trunk_eligible(d) ? SISR_ROUTE_TRUNK : SISR_ROUTE_GENERIC;
}

// rows of stat_part / cnt_part (or bnb_part) a launch of this descriptor writes: the trunk kernel writes one per
// workgroup, the generic kernels (and the last conv's, which has neither epilogue) one per tile (plan.n_tiles)
extern "C" int sisr_conv2d_bf16_parts(const SisrConvDesc* d) {
    if (!d) return SISR_E_BADARG;
    switch (sisr_conv2d_bf16_route(d)) {
        case SISR_ROUTE_DEEP: return sisr_conv2d_deep_parts(d);
        case SISR_ROUTE_TRUNK: return sisr_conv2d_trunk_grid(d);
        default: return d->plan.n_tiles;
    }
}

extern "C" int sisr_conv2d_bf16(const SisrConvDesc* d, void* stream) {
    if (!d || !d->x1 || !d->y) return SISR_E_BADARG;
    const int32_t route = sisr_conv2d_bf16_route(d);
    // the split-K implicit-GEMM family (conv_deep.hip): a descriptor planned for it carries that family's weight image and
    // NOT the generic one, so it either runs there or is refused -- never silently on another kernel
    if (route == SISR_ROUTE_DEEP) {
        if (!sisr_conv2d_deep_eligible(d)) return SISR_E_UNSUPPORTED;
        return sisr_conv2d_deep_launch(d, sisr_stream(stream));
    }
    if (!d->wpk) return SISR_E_BADARG;
    if (operand_needs_x2(d->pro_mode) && !d->x2) return SISR_E_BADARG;
    if (d->stat_part && (!d->cnt_part || d->y_mode != SISR_Y_NHWC)) return SISR_E_BADARG;
    if (d->y_bf16 && (d->y_mode == SISR_Y_NCHW || (d->Cout & 7) || d->epi_act != SISR_EPI_NONE ||
                      (d->y_mode == SISR_Y_NHWC_SHUFFLE2 && ((d->Cout >> 2) & 7)) || (d->res && !d->res_bf16) ||
                      (d->bnb_part && !d->bnbx_bf16) || (d->res && d->y_mode != SISR_Y_NHWC)))
        return SISR_E_UNSUPPORTED;
    if (!d->y_bf16 && ((d->res && d->res_bf16) || (d->bnb_part && d->bnbx_bf16))) return SISR_E_UNSUPPORTED;
    if (d->bnb_part && (d->y_mode != SISR_Y_NHWC || d->y_sy != 1 || d->y_sx != 1 || d->y_H != d->Ho || d->y_W != d->Wo ||
                        !d->bnb_x || !d->bnb_scale || !d->bnb_shift || !d->bnb_mean || !d->bnb_invstd ||
                        d->epi_act != SISR_EPI_NONE || d->plan.CoutPad / (d->plan.nsub * 32) != 1))
        return SISR_E_UNSUPPORTED;
    const SisrConvPlan& p = d->plan;
    if (d->x_mode == SISR_X_NCHW || (d->Cin % BF_CK) || (d->x_mode == SISR_X_NHWC_UNSHUFFLE2 && ((d->Cin >> 2) & 3)))
        return SISR_E_UNSUPPORTED;
    if (p.CK != BF_CK || p.PS != BF_PS || p.n_tiles <= 0 || p.lds_bytes <= 0 || p.lds_bytes > 160 * 1024)
        return SISR_E_BADARG;
    hipStream_t st = sisr_stream(stream);
    if (route == SISR_ROUTE_TOIMAGE) return sisr_conv2d_toimage_launch(d, st);
    if (route == SISR_ROUTE_TRUNK) return sisr_conv2d_trunk_launch(d, st);
    if (d->pro_mode == SISR_PRO_RES_AFFINE) return SISR_E_UNSUPPORTED;      // persistent trunk kernels only
    // TAG only names the symbol (same code): 1 = the generator's trunk geometry in its forward role (BatchNorm
    // statistics epilogue) -- the launch bench.py's roofline probe times --, 2 = the trunk geometry in its other
    // roles (data gradients), 0 = everything else; profiles then report the roles separately
    const bool trunk = d->Cin == 64 && d->Cout == 64 && d->KH == 3 && d->KW == 3 && d->stride == 1;
    const int tag = !trunk ? 0 : (d->stat_part ? 1 : 2);
    if (p.msub == 2 && p.nsub == 2) return launch_conv_bf16<2, 2, 0>(d, st);
    if (p.msub == 2 && p.nsub == 1) return launch_conv_bf16<2, 1, 0>(d, st);
    if (p.msub == 1 && p.nsub == 2)
        return tag == 1 ? launch_conv_bf16<1, 2, 1>(d, st) : tag == 2 ? launch_conv_bf16<1, 2, 2>(d, st) : launch_conv_bf16<1, 2, 0>(d, st);
    if (p.msub == 1 && p.nsub == 1) return launch_conv_bf16<1, 1, 0>(d, st);
    return SISR_E_BADARG;
}
