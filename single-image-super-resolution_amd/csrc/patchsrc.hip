// patchsrc.hip -- device-resident patch source: the decoded dataset stays in HBM -- [M][H0][W0][C] uint8, or
// M images of their own sizes packed into one buffer behind a table of SisrImageRec -- and every iteration's batch is sampled from
// it on the device -- which image, which crop window, which of the eight flips / transpositions -- so a captured iteration needs
// no host gather and no host-to-device copy.
//   patch_draw_kernel    one workgroup: step count t (device memory) -> draw table [B][4] = { index, y0, x0, ops }, t -> t + 1;
//   patch_gather_kernel  one workgroup per 32 x 32 window tile and sample: rows of the window -> LDS -> the flipped / transposed
//                        tile of the destination, normalised fp32 NCHW (ToTensor + Normalize) or uint8 NHWC.
// The random numbers are Philox4x32-10 (Salmon et al., SC'11) keyed by the seed and counted by (t, b, rank): one text for host
// and device (sisr_patch_draws_host is the same arithmetic without a GPU).  No atomics, plain vector stores, nothing read back.
#include "sisr_dev.h"
#include "sisr_philox.h"

#include <algorithm>

#define PATCH_ORDER_RANDOM 0
#define PATCH_ORDER_SEQUENTIAL 1
#define PATCH_ORDER_PERMUTED 2

struct PatchDrawArgs {
    uint64_t seed;
    int rank, world, order, B, M, H0, W0, h, w, ops_mask;
};

// sigma_e(x): the swap-or-not shuffle (Hoang, Morris, Rogaway, CRYPTO 2012) of [0, M), keyed by the seed and the epoch e alone.
// Round r pairs x with its partner x' = K_r - x (mod M) and one bit, drawn for the pair's larger member, decides whether the two
// trade places: an involution per round, so a bijection for every M, with a fixed trip count.  Both draws are counted by the epoch
// in place of the step and tagged DRAW_TAG_PERM_KEY / DRAW_TAG_PERM_BIT - r (sisr_philox.h): no word is shared with a sample's draw.
// K_r belongs to the epoch, not to x: patch_perm_key is computed once per round (ks[r]) and every position walks the same 24.
__host__ __device__ __forceinline__ uint32_t patch_perm_key(uint64_t seed, int64_t e, uint32_t r, uint32_t M) {
    uint32_t o[4];
    draw_words(seed, e, r, DRAW_TAG_PERM_KEY, o);
    return patch_mulhi32(o[0], M);
}

__host__ __device__ __forceinline__ uint32_t patch_permute(uint64_t seed, int64_t e, const uint32_t* ks, uint32_t x, uint32_t M) {
    for (uint32_t r = 0; r < PATCH_PERM_ROUNDS; ++r) {
        uint32_t xp = ks[r] + M - x;                 // in [1, 2 M): M < 2^31, no wrap
        if (xp >= M) xp -= M;
        uint32_t o[4];
        draw_words(seed, e, xp > x ? xp : x, DRAW_TAG_PERM_BIT - r, o);
        if (o[0] & 1u) x = xp;
    }
    return x;
}

// batches per epoch of the sequential and permuted orders (drop_last)
__host__ __device__ __forceinline__ int64_t patch_epoch_batches(const PatchDrawArgs& a) { return (int64_t)a.M / ((int64_t)a.B * a.world); }

// row b of the draw table of step t.  Multiply-high maps a 32-bit word onto [0, range): no rejection loop, bias <= range / 2^32.
// table: the drawn image's own H and W bound the offsets (NULL: every image is H0 x W0); an image smaller than the window, which
// the host refuses where it can see the table, has range 1.  ks: the round keys of step t's epoch, read in permuted order only
__host__ __device__ __forceinline__ void patch_draw_row(const PatchDrawArgs& a, const SisrImageRec* table, const uint32_t* ks,
                                                        int64_t t, int b, int32_t* row) {
    uint32_t r[4];
    draw_words(a.seed, t, (uint32_t)b, (uint32_t)a.rank, r);
    int32_t index;
    if (a.order == PATCH_ORDER_RANDOM) {
        index = (int32_t)patch_mulhi32(r[0], (uint32_t)a.M);
    } else {                                       // SamplerRange(0, M) with drop_last, restarting each epoch ...
        const int64_t nb = patch_epoch_batches(a);
        index = (int32_t)(((t % nb) * a.world + a.rank) * a.B + b);
        if (a.order == PATCH_ORDER_PERMUTED)       // ... read through the epoch's permutation
            index = (int32_t)patch_permute(a.seed, t / nb, ks, (uint32_t)index, (uint32_t)a.M);
    }
    const int ry = (table ? table[index].H : a.H0) - a.h + 1, rx = (table ? table[index].W : a.W0) - a.w + 1;
    row[0] = index;
    row[1] = (int32_t)patch_mulhi32(r[1], (uint32_t)(ry > 1 ? ry : 1));
    row[2] = (int32_t)patch_mulhi32(r[2], (uint32_t)(rx > 1 ? rx : 1));
    row[3] = (int32_t)(r[3] & (uint32_t)a.ops_mask);
}

// has_table: H0 and W0 are not read.  permuted: whether the entry point knows order 2
static bool patch_draw_args_ok(const PatchDrawArgs& a, bool has_table, bool permuted) {
    if (a.B <= 0 || a.M <= 0 || a.h <= 0 || a.w <= 0) return false;
    if (!has_table && (a.H0 <= 0 || a.W0 <= 0 || a.h > a.H0 || a.w > a.W0)) return false;
    if (a.world <= 0 || a.rank < 0 || a.rank >= a.world) return false;
    if (a.ops_mask < 0 || a.ops_mask > 7 || ((a.ops_mask & 4) && a.h != a.w)) return false;
    if (a.order == PATCH_ORDER_SEQUENTIAL || (permuted && a.order == PATCH_ORDER_PERMUTED))
        return patch_epoch_batches(a) >= 1;                                                          // an epoch of no batch: refused
    return a.order == PATCH_ORDER_RANDOM;
}

// One workgroup, the step protocol of sisr_philox.h.  Permuted order: 24 threads leave the epoch's round keys in LDS before its barrier.
__global__ void __launch_bounds__(SISR_BLOCK) patch_draw_kernel(int64_t* __restrict__ step, PatchDrawArgs a,
                                                                 const SisrImageRec* __restrict__ table, int32_t* __restrict__ draws) {
    __shared__ uint32_t ks[PATCH_PERM_ROUNDS];
    const int64_t t = draw_step_read(step);
    if (a.order == PATCH_ORDER_PERMUTED && threadIdx.x < PATCH_PERM_ROUNDS)
        ks[threadIdx.x] = patch_perm_key(a.seed, t / patch_epoch_batches(a), threadIdx.x, (uint32_t)a.M);
    draw_step_advance(step, t, nullptr);
    for (int b = threadIdx.x; b < a.B; b += SISR_BLOCK) {
        int32_t row[4];
        patch_draw_row(a, table, ks, t, b, row);
        draws[4 * b + 0] = row[0]; draws[4 * b + 1] = row[1]; draws[4 * b + 2] = row[2]; draws[4 * b + 3] = row[3];
    }
}

// ---- gather ----------------------------------------------------------------------------------------------------------------------
// Tile: PG_T x PG_T window pixels.  A window row is w * C contiguous bytes at an arbitrary byte offset and the destination is
// planar, so neither side can be both read and written in its own order by one thread mapping: the tile's rows are copied to LDS
// byte for byte (consecutive lanes on consecutive source bytes) and read back in DESTINATION order (consecutive lanes on
// consecutive destination elements), whichever of the eight operations applies.  LDS pitch PG_PITCH = 132 bytes = 33 dwords: a
// transposed read walks DOWN a tile column, one row per lane, and 33 is odd, so the 32 lanes of a half-wave fall on 32 different
// banks; an untransposed read walks along a row (stride C bytes: lanes share dwords or take neighbouring ones).
#define PG_T 32
#define PG_PITCH (PG_T * 4 + 4)

// TABLE: image `index` is table[index].H x table[index].W at byte table[index].offset of `data` (H0, W0 unused); a byte whose
// offset is not inside [0, data_bytes) is not loaded and reads as 0, whatever the table holds.  Offsets are 64-bit throughout.
template <int KIND, bool TABLE>
__global__ void __launch_bounds__(SISR_BLOCK) patch_gather_kernel(const unsigned char* __restrict__ data, int64_t data_bytes,
                                                                   const SisrImageRec* __restrict__ table, int M, int H0, int W0, int C,
                                                                   const int32_t* __restrict__ draws, int h, int w, float mean,
                                                                   float stdv, void* __restrict__ dst) {
    __shared__ unsigned char tile[PG_T * PG_PITCH];
    const int b = blockIdx.z;
    // a table can never make the kernel read outside `data` or write outside `dst`: every entry is clamped into range
    const int index = min(max(draws[4 * b + 0], 0), M - 1);
    int64_t base = 0;
    if (TABLE) {
        const SisrImageRec rec = table[index];
        base = rec.offset; H0 = rec.H; W0 = rec.W;
    }
    const int y0 = max(min(draws[4 * b + 1], H0 - h), 0);
    const int x0 = max(min(draws[4 * b + 2], W0 - w), 0);
    int ops = draws[4 * b + 3] & 7;
    if (h != w) ops &= 3;
    const bool fh = ops & 1, fv = ops & 2, tr = ops & 4;
    const int ty0 = blockIdx.y * PG_T, tx0 = blockIdx.x * PG_T;          // tile origin inside the window
    const int th = min(PG_T, h - ty0), tw = min(PG_T, w - tx0);          // ragged last tiles
    const int rowbytes = tw * C;
    const int64_t src_pitch = (int64_t)W0 * C;
    if (TABLE) {
        const int64_t first = base + ((int64_t)(y0 + ty0) * W0 + x0 + tx0) * C;
        for (int i = threadIdx.x; i < th * rowbytes; i += SISR_BLOCK) {
            const int r = i / rowbytes, j = i - r * rowbytes;
            const int64_t at = first + r * src_pitch + j;
            tile[r * PG_PITCH + j] = at >= 0 && at < data_bytes ? data[at] : (unsigned char)0;
        }
    } else {
        const unsigned char* src = data + (((int64_t)index * H0 + y0 + ty0) * W0 + x0 + tx0) * C;
        for (int i = threadIdx.x; i < th * rowbytes; i += SISR_BLOCK) {
            const int r = i / rowbytes, j = i - r * rowbytes;
            tile[r * PG_PITCH + j] = src[r * src_pitch + j];
        }
    }
    __syncthreads();
    // the tile after hflip, vflip: rows [yb, yb + th), columns [xb, xb + tw) of the flipped window; after the transposition
    // its rows are the flipped window's columns
    const int yb = fv ? h - ty0 - th : ty0, xb = fh ? w - tx0 - tw : tx0;
    const int OH = tr ? w : h, OW = tr ? h : w;
    const int on = tr ? tw : th, om = tr ? th : tw;                      // rows, columns of the destination tile
    const int oy0 = tr ? xb : yb, ox0 = tr ? yb : xb;
    if (KIND == 0) {
        float* out = reinterpret_cast<float*>(dst) + (int64_t)b * C * OH * OW;
        const int q = threadIdx.x & (PG_T - 1);
        if (q < om) {
            for (int r = threadIdx.x / PG_T; r < on; r += SISR_BLOCK / PG_T) {
                const int ly = tr ? q : r, lx = tr ? r : q;
                const int lsy = fv ? th - 1 - ly : ly, lsx = fh ? tw - 1 - lx : lx;
                const unsigned char* px = tile + lsy * PG_PITCH + lsx * C;
                float* o = out + (int64_t)(oy0 + r) * OW + ox0 + q;
                for (int c = 0; c < C; ++c) {
                    const float t = (float)px[c] / 255.0f;                   // ToTensor (correctly rounded division)
                    o[(int64_t)c * OH * OW] = (t - mean) / stdv;             // Normalize: the expressions of resize_u8_normalize_kernel
                }
            }
        }
    } else {
        unsigned char* out = reinterpret_cast<unsigned char*>(dst) + (int64_t)b * OH * OW * C;
        const int orow = om * C;
        for (int i = threadIdx.x; i < on * orow; i += SISR_BLOCK) {
            const int r = i / orow, jb = i - r * orow;
            const int q = jb / C, c = jb - q * C;
            const int ly = tr ? q : r, lx = tr ? r : q;
            const int lsy = fv ? th - 1 - ly : ly, lsx = fh ? tw - 1 - lx : lx;
            out[((int64_t)(oy0 + r) * OW + ox0) * C + jb] = tile[lsy * PG_PITCH + lsx * C + c];
        }
    }
}

// ---- entry points ----------------------------------------------------------------------------------------------------------------
static int patch_draws_host(const PatchDrawArgs& a, const SisrImageRec* table_host, bool permuted, int64_t t, int32_t* draws_host) {
    if (!draws_host || t < 0 || !patch_draw_args_ok(a, table_host != nullptr, permuted)) return SISR_E_BADARG;
    if (table_host)
        for (int i = 0; i < a.M; ++i)
            if (table_host[i].H < a.h || table_host[i].W < a.w) return SISR_E_BADARG;
    uint32_t ks[PATCH_PERM_ROUNDS] = {};
    if (a.order == PATCH_ORDER_PERMUTED)
        for (uint32_t r = 0; r < PATCH_PERM_ROUNDS; ++r) ks[r] = patch_perm_key(a.seed, t / patch_epoch_batches(a), r, (uint32_t)a.M);
    for (int b = 0; b < a.B; ++b) patch_draw_row(a, table_host, ks, t, b, draws_host + 4 * (int64_t)b);
    return 0;
}

static int patch_draw_launch(int64_t* step_dev, const PatchDrawArgs& a, const SisrImageRec* table_dev, bool permuted,
                             int32_t* draws_dev, void* stream) {
    if (!step_dev || !draws_dev || !patch_draw_args_ok(a, table_dev != nullptr, permuted)) return SISR_E_BADARG;
    hipLaunchKernelGGL(patch_draw_kernel, dim3(1), dim3(SISR_BLOCK), 0, sisr_stream(stream), step_dev, a, table_dev, draws_dev);
    SISR_CHECK_LAUNCH();
    return 0;
}

extern "C" int sisr_patch_draws_host(int64_t t, uint64_t seed, int32_t rank, int32_t world, int32_t order, int32_t B, int32_t M,
                                     int32_t H0, int32_t W0, int32_t h, int32_t w, int32_t ops_mask, int32_t* draws_host) {
    return patch_draws_host({seed, rank, world, order, B, M, H0, W0, h, w, ops_mask}, nullptr, false, t, draws_host);
}

extern "C" int sisr_patch_draws_table_host(int64_t t, uint64_t seed, int32_t rank, int32_t world, int32_t order, int32_t B,
                                           int32_t M, int32_t H0, int32_t W0, const SisrImageRec* table_host, int32_t h, int32_t w,
                                           int32_t ops_mask, int32_t* draws_host) {
    return patch_draws_host({seed, rank, world, order, B, M, H0, W0, h, w, ops_mask}, table_host, true, t, draws_host);
}

extern "C" int sisr_patch_draw(int64_t* step_dev, uint64_t seed, int32_t rank, int32_t world, int32_t order, int32_t B, int32_t M,
                               int32_t H0, int32_t W0, int32_t h, int32_t w, int32_t ops_mask, int32_t* draws_dev, void* stream) {
    return patch_draw_launch(step_dev, {seed, rank, world, order, B, M, H0, W0, h, w, ops_mask}, nullptr, false, draws_dev, stream);
}

extern "C" int sisr_patch_draw_table(int64_t* step_dev, uint64_t seed, int32_t rank, int32_t world, int32_t order, int32_t B,
                                     int32_t M, int32_t H0, int32_t W0, const SisrImageRec* table_dev, int32_t h, int32_t w,
                                     int32_t ops_mask, int32_t* draws_dev, void* stream) {
    return patch_draw_launch(step_dev, {seed, rank, world, order, B, M, H0, W0, h, w, ops_mask}, table_dev, true, draws_dev, stream);
}

template <bool TABLE>
static int patch_gather_launch(const unsigned char* data, int64_t data_bytes, const SisrImageRec* table_dev, int M, int H0, int W0,
                               int C, const int32_t* draws_dev, int B, int h, int w, float mean, float stdv, void* dst, int dst_kind,
                               void* stream) {
    const int tiles_x = (w + PG_T - 1) / PG_T, tiles_y = (h + PG_T - 1) / PG_T;
    if (B > 65535 || tiles_y > 65535) return SISR_E_TOOBIG;
    const dim3 grid(tiles_x, tiles_y, B);
    if (dst_kind == 0)
        hipLaunchKernelGGL((patch_gather_kernel<0, TABLE>), grid, dim3(SISR_BLOCK), 0, sisr_stream(stream), data, data_bytes,
                           table_dev, M, H0, W0, C, draws_dev, h, w, mean, stdv, dst);
    else
        hipLaunchKernelGGL((patch_gather_kernel<1, TABLE>), grid, dim3(SISR_BLOCK), 0, sisr_stream(stream), data, data_bytes,
                           table_dev, M, H0, W0, C, draws_dev, h, w, mean, stdv, dst);
    SISR_CHECK_LAUNCH();
    return 0;
}

extern "C" int sisr_patch_gather(const unsigned char* data, int32_t M, int32_t H0, int32_t W0, int32_t C, const int32_t* draws_dev,
                                 int32_t B, int32_t h, int32_t w, float mean, float stdv, void* dst, int32_t dst_kind, void* stream) {
    if (!data || !draws_dev || !dst || M <= 0 || H0 <= 0 || W0 <= 0 || C < 1 || C > 4 || B <= 0 || h <= 0 || w <= 0 || h > H0 ||
        w > W0 || (dst_kind != 0 && dst_kind != 1) || (dst_kind == 0 && !(stdv != 0.f)))
        return SISR_E_BADARG;
    return patch_gather_launch<false>(data, 0, nullptr, M, H0, W0, C, draws_dev, B, h, w, mean, stdv, dst, dst_kind, stream);
}

extern "C" int sisr_patch_gather_table(const unsigned char* data, int64_t data_bytes, const SisrImageRec* table_dev, int32_t M,
                                       int32_t C, const int32_t* draws_dev, int32_t B, int32_t h, int32_t w, float mean, float stdv,
                                       void* dst, int32_t dst_kind, void* stream) {
    if (!data || data_bytes < 1 || !table_dev || !draws_dev || !dst || M <= 0 || C < 1 || C > 4 || B <= 0 || h <= 0 || w <= 0 ||
        (dst_kind != 0 && dst_kind != 1) || (dst_kind == 0 && !(stdv != 0.f)))
        return SISR_E_BADARG;
    return patch_gather_launch<true>(data, data_bytes, table_dev, M, 0, 0, C, draws_dev, B, h, w, mean, stdv, dst, dst_kind, stream);
}
