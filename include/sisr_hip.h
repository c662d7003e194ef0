/*
 * sisr_hip.h -- C ABI of libsisr_hip.so: the MI355X (gfx950) kernels behind the SRGAN hot path
 * of keyber/Single-Image-Super-Resolution.
 *
 * The reference has no FFI of its own: its boundary is the Python nn.Module API
 * (model_generator.py:22-141, model_discriminator.py:18-76, model_content_extractor.py:33-60,
 * utils.py:16-31) and every FLOP runs inside torch.nn primitives.  Each entry point below
 * replaces the torch primitive call sites listed next to it; the Python host side
 * (single-image-super-resolution_amd/) binds them with ctypes and re-creates the reference's
 * module interface on top.
 *
 * Conventions
 *   - plain pointers and sizes only; all pointers are DEVICE pointers unless named host_*;
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*), allocates nothing,
 *     and returns 0 on success or a hipError_t / negative SISR_E* code; it never aborts;
 *   - activations are NHWC fp32 inside the path; NCHW (the reference's layout) is accepted on the
 *     3-channel image side and produced on the RGB / feature-tap side by layout flags;
 *   - descriptors are filled by the caller for geometry, then completed by the matching
 *     *_plan() call which chooses the tiling and reports workspace sizes.
 */
#ifndef SISR_HIP_H
#define SISR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SISR_E_BADARG (-1)
#define SISR_E_TOOBIG (-2)
#define SISR_E_UNSUPPORTED (-3)

/* ---- input-operand ("prologue") modes: the value fed to the contraction for input element
 *      (n,iy,ix,c); x1/x2 share shape and layout; out-of-image taps contribute 0. ------------- */
enum {
    SISR_PRO_NONE = 0,        /* v = x1                                                        */
    SISR_PRO_ACT = 1,         /* v = lrelu(x1, slope)            PReLU / LeakyReLU / ReLU       */
    SISR_PRO_AFFINE_ACT = 2,  /* v = lrelu(pa[c]*x1 + pd[c], slope)   BatchNorm apply + act     */
    SISR_PRO_BNBWD = 3,       /* v = pa[c]*x1 + pb[c]*x2 + pd[c]      BatchNorm backward        */
    SISR_PRO_BNACT_BWD = 4,   /* z = ps[c]*x2+pt[c]; g = z>0 ? x1 : slope*x1;
                                 v = pa[c]*g + pb[c]*x2 + pd[c]       act' then BatchNorm bwd   */
    SISR_PRO_ACT_BWD = 5,     /* v = x2>0 ? x1 : slope*x1             act' (x2 = pre-activation)*/
    SISR_PRO_TANH_BWD = 6,    /* v = x1*(1 - x2*x2)                   tanh' (x2 = tanh output)  */
    SISR_PRO_RES_AFFINE = 7   /* v = lrelu(x1, slope) + (pa[c]*x2 + pd[c])   residual-block skip sum x + BN2(c2)
                                 (model_generator.py:19) formed in the consuming conv's staging; the sum is also
                                 stored to x_out once per pixel.  Persistent trunk kernels only (forward role):
                                 the generic kernels return SISR_E_UNSUPPORTED. */
};
enum { SISR_X_NHWC = 0, SISR_X_NCHW = 1, SISR_X_NHWC_UNSHUFFLE2 = 2 };
enum { SISR_Y_NHWC = 0, SISR_Y_NCHW = 1, SISR_Y_NHWC_SHUFFLE2 = 2 };
enum { SISR_EPI_NONE = 0, SISR_EPI_TANH = 1 };

/* Packed-weight layout shared by conv / wgrad / weight kernels:
 *   wpk[chunk][r][co][krow], krow = s*PS + (ci - chunk*CK), row length KROWP (zero padded),
 *   co < CoutPad (zero padded).  PS = CK|1 keeps LDS reads conflict-free. */
typedef struct SisrConvPlan {
    int32_t TH, TW, TN;             /* output tile: TN images x TH x TW pixels               */
    int32_t tiles_y, tiles_x, n_groups, n_tiles;
    int32_t CK, PS, KROWP, n_chunk, CoutPad;
    int32_t msub, nsub;             /* 32x32 MFMA sub-tiles per wave (M) / per block (N)     */
    int32_t lds_bytes;
    int32_t wpk_elems;              /* elements in the packed weight buffer                  */
    int32_t variant;                /* bf16 family, bit 0: the weight buffer carries the LANE-ORDER image of the persistent trunk
                                       kernels behind the standard one (SISR_WIMG_BF16, extra); fp32 family, bits 1-2:
                                       the LDS-order image behind the standard one (SISR_WIMG_F32, extra: 2 = fp32
                                       values, 4 = split pairs; used only when it matches mfma_split); set by the caller on the
                                       descriptor it launches, 0 after planning                                  */
    /* bf16 family: reciprocals m = ceil(2^32 / d) (0 for d = 1) so that n / d = umulhi(n, m) for n, d < 2^16 --
     * the kernels' index arithmetic (tile id, tile row, LDS row) without integer division */
    uint32_t m_tiles_x, m_thw, m_tw, m_iw, m_wrow;
} SisrConvPlan;

/* Plan of the split-K implicit-GEMM kernels of conv_deep.hip (bf16 build; filled by sisr_conv2d_deep_plan): the layers whose
 * contraction is deep and whose images are small -- the discriminator's strided-conv stack (model_discriminator.py:10,39-44), the
 * VGG19 feature convs (model_content_extractor.py:43) and the generator's trunk at sizes the persistent trunk kernels do not take.
 * A workgroup owns 128 output pixels x BN output channels x one K slice (a range of 32-channel chunks); an output tile is TH rows of
 * the FLATTENED (image, output row) space x TW columns, so that a band of full-width rows may straddle images (12 x 12 and 6 x 6 maps
 * fill 120 / 126 of the 128 MFMA rows); with split > 1 every workgroup leaves its fp32 partial tile in `ws` and
 * conv_deep_finish_kernel sums the slices in a fixed order and runs the epilogue (bias, statistics, reductions, bf16 store). */
typedef struct SisrDeepPlan {
    int32_t enabled;                /* 1: sisr_conv2d_bf16 runs this descriptor on conv_deep.hip            */
    int32_t TH, TW;                 /* output tile: TH flattened output rows x TW columns (<= 128 pixels)   */
    int32_t tiles_x, tiles_q;       /* column tiles, row-band tiles                                         */
    int32_t BN, n_ntiles;           /* output channels per workgroup (64 | 128), cout tiles                 */
    int32_t n_chunk, split, cps;    /* 32-channel chunks, K slices, chunks per slice                        */
    int32_t PR;                     /* padded input rows per image (pad_y + H + bottom padding)             */
    int32_t IW, IH_max;             /* halo tile: columns, most rows of any tile                            */
    int32_t NIT;                    /* 16-byte staging items per thread                                     */
    int32_t wimg_elems;             /* bf16 elements of the weight image [chunk][tap row][Cout][KW*32 + 8]  */
    int32_t classes;                /* 1, or 4: the output-parity classes of a stride-2 data gradient in ONE launch   */
    int64_t ws_bytes;               /* bytes of the split workspace (0 when split == 1)                     */
    uint32_t m_tiles_x, m_tw, m_ho, m_pr, m_iw;
    uint32_t rsv2;
} SisrDeepPlan;

/* Direct convolution, fp32 storage, fp32 MFMA (v_mfma_f32_32x32x2_f32) accumulate.
 * Replaces nn.Conv2d forward and its data-gradient (model_generator.py:10,13,33,39,45,52,123;
 * model_discriminator.py:10,39; torchvision VGG19 convs via model_content_extractor.py:43) with
 * the neighbouring BatchNorm2d-apply / PReLU / LeakyReLU / ReLU (prologue), bias, Tanh,
 * PixelShuffle(2) and residual add (epilogue) and the BatchNorm batch statistics fused in. */
typedef struct SisrConvDesc {
    const float *x1, *x2;                    /* input operand(s)                              */
    const float *pa, *pb, *pd, *ps, *pt;     /* per-input-channel prologue constants          */
    const float *wpk;                        /* packed weights (see above)                    */
    const float *bias;                       /* [Cout] in ORIGINAL channel order, or NULL     */
    const float *res;                        /* residual, same layout as y, or NULL           */
    float *y;
    float *stat_part;                        /* [n_tiles][2][Cout] (mean, M2) or NULL         */
    float *cnt_part;                         /* [n_tiles] valid pixels per tile               */
    /* bf16 kernels, NHWC output: the output y is the gradient g arriving at a BatchNorm (optionally through the
     * leaky activation after it); the epilogue then also emits that BatchNorm's backward reductions per tile --
     * bnb_part[tile][0..C) = sum gg, [C..2C) = sum gg*xhat, [2C] = sum_{z<=0} g*z  (gg = act'(z)*g,
     * z = scale*x + shift, xhat = (x - mean)*invstd) -- in the row format sisr_bn_bwd_finalize reads.  NULL: off. */
    const float *bnb_x, *bnb_scale, *bnb_shift, *bnb_mean, *bnb_invstd;
    const float *bnb_slope_p;
    float *bnb_part;
    float *x_out;                            /* SISR_PRO_RES_AFFINE: the materialised operand, layout / type of x1 */
    /* Deferred BatchNorm finalisation (persistent forward trunk kernels, prologues AFFINE_ACT / RES_AFFINE): when
     * fin_stat is set, pa / pd are NOT read -- every workgroup merges the fin_rows statistics rows (fin_stat [rows][2][Cin]
     * mean / M2, fin_cnt [rows]) of the BatchNorm whose apply the prologue is, exactly as sisr_bn_finalize does (Chan's
     * formula in double), and uses scale = gamma * invstd, shift = beta - mean * scale; workgroup 0 also writes
     * fin_k [4][Cin] = scale, shift, mean, invstd and updates the running statistics (momentum, unbiased variance).
     * Saves the 5-6 us sisr_bn_finalize launch between two convs. */
    const float *fin_stat, *fin_cnt, *fin_gamma, *fin_beta;
    float *fin_rm, *fin_rv, *fin_k;
    int32_t N, H, W, Cin;                    /* logical input                                 */
    int32_t Ho, Wo, Cout;                    /* logical output grid                           */
    int32_t KH, KW, stride, pad_y, pad_x;
    int32_t x_mode, pro_mode;
    const float *pro_slope_p;                /* device scalar slope (PReLU weight); NULL: pro_slope */
    float pro_slope;
    int32_t y_mode, epi_act;
    int32_t bnb_act; float bnb_slope;        /* activation after that BatchNorm: 0 none, 1 leaky (slope / *slope_p) */
    int32_t y_sy, y_oy, y_sx, y_ox, y_H, y_W; /* output pixel (oy*y_sy+y_oy, ox*y_sx+y_ox) of a
                                                y_H x y_W image (strided scatter for the data
                                                gradient of stride-2 convs); plain: 1,0,1,0,Ho,Wo */
    /* storage type of the tensors behind the float* fields (0: fp32, 1: bf16 -- the bf16 build keeps NHWC
     * activations and gradients as bf16 in HBM; all arithmetic, accumulation and statistics stay fp32).
     * x_bf16: x1 and x2;  y_bf16: y (NHWC / NHWC_SHUFFLE2 only);  res_bf16: res;  bnbx_bf16: bnb_x. */
    int32_t x_bf16, y_bf16, res_bf16, bnbx_bf16;
    int32_t fin_rows; float fin_momentum, fin_eps;
    /* fp32 tensors, trunk geometry only: 1 = the contraction runs on the bf16 matrix instruction over (hi, lo) bf16 pairs of every
     * fp32 operand (hi*hi + hi*lo + lo*hi, fp32 accumulate; operands good to 2^-17 relative); 0 = exact fp32 matrix instruction */
    int32_t mfma_split;
    SisrConvPlan plan;
    /* conv_deep.hip (see SisrDeepPlan): `wdeep` = the weight image in that family's layout (SISR_WIMG_DEEP),
     * `deep_ws` = the caller's split workspace (deep.ws_bytes; may be NULL when deep.split == 1), `epi_scale_p` = device scalar the
     * accumulators are multiplied by before the bias (1 / sigma of a spectrally normalised weight packed un-normalised) or NULL */
    const void *wdeep;
    float *deep_ws;
    const float *epi_scale_p;
    /* deep.classes == 4 -- the data gradient of a stride-2 3x3 convolution (even H, W) as ONE launch over its four output-parity
     * classes c = 2 py + px: the descriptor describes the class convolution with the MOST taps (KH = KW = 2, stride 1, pad 0, over
     * dy; Ho x Wo = the class grid H/2 x W/2; y_sy = y_sx = 2, y_H x y_W = the gradient's size); class c has deep_ckh[c] tap rows,
     * writes output pixel (2 a + py, 2 b + px) and reads its weights from wdeep_c[c] -- always in the KW = 2 row format, a class
     * with one tap per row carries zeros for the second (SISR_WIMG_DEEP with extra = 2).  Partial rows (bnb_part) and split
     * workspace tiles are class-major. */
    const void *wdeep_c[4];
    int32_t deep_ckh[4];
    SisrDeepPlan deep;
} SisrConvDesc;

int sisr_conv2d_plan(SisrConvDesc *d);                        /* host only: fills d->plan     */
int sisr_conv2d_f32(const SisrConvDesc *d, void *stream);

/* Weight gradient of the same convolution: dW[r][s][ci][co] = sum_pix in(pix+tap)[ci]*dy(pix)[co].
 * Replaces the weight/bias part of convolution_backward for the call sites above.  The input
 * operand (x*, p*, x_mode, pro_*) and the output-gradient operand (g*, q*, g_mode, gpro_*) take
 * the same prologue modes.  Each block writes one fp32 partial slab; sisr_wgrad_reduce sums them. */
/* Plan of wgrad_deep.hip (bf16 build, filled by sisr_wgrad_deep_plan after sisr_wgrad_plan_bf16): the weight gradient of the 3x3
 * layers with channels in 64s (the discriminator's conv stack, the generator's trunk at sizes the persistent kernel does not take).
 * A workgroup owns 64 input channels x 64 output channels x all 9 taps (nine 32 x 32 accumulators per wave: the whole block of the
 * gradient stays in registers over all of the workgroup's pixel tiles) and a share of the pixel tiles; the tiles are conv_deep.hip's
 * (rows of the flattened (image, row) space, so 6 x 6 .. 24 x 24 maps waste no MFMA rows), the contraction runs over the tile's
 * positions in HALO coordinates -- dy is laid out on the pitch of the x halo, so that tap (ky, kx) is the x image shifted by a
 * constant -- and both operands are staged one tile ahead. */
typedef struct SisrWgradDeepPlan {
    int32_t enabled;
    int32_t TH, TW, tiles_x, tiles_q, n_tiles;
    int32_t PR;                     /* padded x rows per image                                                   */
    int32_t IW, IH_max;             /* x halo: pitch (even for stride 2), most rows of any tile                  */
    int32_t IWd, IHd_max;           /* dy image in halo coordinates: pitch (IW, or IW / 2 for stride 2), rows    */
    int32_t NPOS_max;               /* positions of the contraction per tile, a multiple of 16                   */
    int32_t XP_max;                 /* x halo pixels incl. the slack the last K step reads                       */
    int32_t NITX, NITD;             /* 16-byte staging items per thread (x, dy)                                  */
    int32_t n_pb, tiles_per_pb;     /* pixel blocks (= slabs) and tiles per block                                */
    int32_t n_cib, n_cob;           /* 64-channel blocks of Cin / Cout                                           */
    int32_t lds_bytes;
    int32_t slab_bf16;              /* the gradient part of a slab row is bf16 (sisr_wgrad_bf16_slab_lead)       */
    int32_t batch_first_wg;         /* sisr_wgrad_deep_batch: first flat workgroup index of this member (0 alone) */
    uint32_t m_tiles_x, m_tw, m_ho, m_pr, m_iw, m_iwd;
} SisrWgradDeepPlan;

typedef struct SisrWgradDesc {
    const float *x1, *x2, *pa, *pb, *pd, *ps, *pt;   /* conv-input operand                    */
    const float *g1, *g2, *qa, *qb, *qd, *qs, *qt;   /* output-gradient operand               */
    float *slab;            /* [n_slabs][slab_stride]: packed dW, layout [chunk][r][krow][co]       */
    float *bias_slab;       /* per-slab bias partial [CoutPad] at the same slab_stride, or NULL
                               (normally slab + slab_elems, slab_stride = slab_elems + CoutPad)    */
    int32_t N, H, W, Cin, Ho, Wo, Cout;
    int32_t KH, KW, stride, pad_y, pad_x;
    int32_t x_mode, pro_mode;
    const float *pro_slope_p;
    float pro_slope;
    int32_t g_mode, gpro_mode;
    const float *gpro_slope_p;
    float gpro_slope;
    /* plan (filled by sisr_wgrad_plan) */
    int32_t TH, TW, TN, tiles_y, tiles_x, n_groups, n_tiles;
    int32_t CK, PS, KROWP, n_chunk, CoutPad;
    int32_t NJ, NP, NT, TSTEP, TVALID;       /* co sub-tiles, pixel parts, row tiles          */
    int32_t grid_x, n_slabs, slab_elems, lds_bytes;
    uint32_t m_tiles_x, m_tiles_y, m_iw, m_twp, m_kw;   /* bf16 kernel: reciprocals as in SisrConvPlan */
    int32_t x_bf16, g_bf16;                  /* storage type of x1/x2 and of g1/g2 (0: fp32, 1: bf16) */
    int32_t mfma_split;                      /* fp32 operands, trunk geometry: as SisrConvDesc.mfma_split */
    int64_t slab_stride;                     /* set by the caller after planning              */
    SisrWgradDeepPlan deep;                  /* wgrad_deep.hip (enabled: sisr_conv2d_wgrad_bf16 runs the descriptor there)  */
} SisrWgradDesc;

int sisr_wgrad_plan(SisrWgradDesc *d, int32_t max_pixel_blocks);
/* bf16 matrix-core variants (v_mfma_f32_32x32x16_bf16, fp32 accumulate; activations fp32 or bf16 in HBM -- see the
 * *_bf16 storage flags -- converted while staged into LDS).  Same descriptors; `wpk` points at the bf16 image written by
 * sisr_weights_prepare (SISR_WIMG_BF16).  Requirements: Cin % 32 == 0, KH*KW <= 9, NHWC
 * operands; SISR_E_UNSUPPORTED otherwise (callers keep the fp32 kernels for those layers). */
int sisr_conv2d_plan_bf16(SisrConvDesc *d);
int sisr_conv2d_bf16(const SisrConvDesc *d, void *stream);
/* conv_deep.hip: fills d->deep for a descriptor whose geometry / modes are set (after sisr_conv2d_plan_bf16); returns
 * SISR_E_UNSUPPORTED (and leaves deep.enabled = 0) for geometries that family does not take: Cin % 32, Cout % 64, taps <= 3 x 3,
 * stride 1 | 2, NHWC bf16 in and out.  target_wg: workgroup slots a launch should fill through the K split (0: default 256).
 * sisr_conv2d_bf16 dispatches to it when deep.enabled && wdeep; sisr_conv2d_bf16_parts counts its partial rows. */
int sisr_conv2d_deep_plan(SisrConvDesc *d, int32_t target_wg, int32_t prefer_bn, int32_t classes);
/* prefer_bn: 0 = choose (64-cout tiles, two workgroups per CU, where there are plenty of pixel tiles; 128 otherwise), 64 | 128 = a
 * caller that knows its prologue is heavy (the two-tensor BatchNorm-backward forms cost ~500 vector instructions per chunk and
 * thread: a 128-cout tile has twice the MFMAs to hide them behind) asks for 128.  classes: 1, or 4 (see SisrConvDesc.wdeep_c). */
/* a fully filled descriptor (storage flags, modes, fusions, wdeep, deep_ws) will run on conv_deep.hip */
int sisr_conv2d_deep_eligible(const SisrConvDesc *d);
/* The generator's trunk geometry (3x3, 64 -> 64, stride 1, bf16 NHWC in and out, H % 8 == 0, W % 16 == 0; forward-type
 * prologue, no residual) runs on a persistent weights-in-registers kernel (conv_trunk.hip) behind sisr_conv2d_bf16;
 * sisr_conv2d_trunk_eligible tells whether a fully filled descriptor will.  That kernel writes ONE statistics partial
 * per workgroup instead of one per tile: sisr_conv2d_bf16_parts(d) = rows of stat_part / cnt_part (bnb_part) the launch
 * of `d` writes -- size those buffers with it (fill geometry, modes, storage flags, res / bnb pointers first). */
int sisr_conv2d_trunk_eligible(const SisrConvDesc *d);
int sisr_conv2d_bf16_parts(const SisrConvDesc *d);
/* The fp32 parity build has its own persistent kernel for that geometry (fp32 NHWC in and out, H % 8 == 0, W % 16 == 0;
 * conv_trunk_f32.hip, behind sisr_conv2d_f32): eligible returns 1 for the forward role, 2 for the data-gradient role;
 * sisr_conv2d_f32_parts(d) = rows of stat_part / cnt_part the launch writes (one per pair of workgroups). */
int sisr_conv2d_trunk_f32_eligible(const SisrConvDesc *d);
int sisr_conv2d_f32_parts(const SisrConvDesc *d);
/* rows of bnb_part (SisrConvDesc.bnb_*: fused BatchNorm-backward reductions) a data-gradient launch of `d` writes through
 * sisr_conv2d_f32 -- one per workgroup of the persistent fp32 trunk kernel; 0 when that kernel does not take `d` (the
 * generic fp32 kernel has no such epilogue: leave bnb_part NULL and run sisr_bn_bwd's own reduction). */
int sisr_conv2d_f32_bnb_parts(const SisrConvDesc *d);
/* bf16 build: the two 9x9 convolutions over a 3-channel NCHW fp32 image that produce 64 bf16 NHWC channels -- the
 * generator's first conv (model_generator.py:33) and the data gradient of its last one (model_generator.py:52, tanh'
 * as prologue) -- run on conv_thin.hip (bf16 MFMA operands like every other layer of that build) behind
 * sisr_conv2d_f32 when H % 16 == W % 16 == 0; tells whether a filled descriptor will. */
int sisr_conv2d_thin_eligible(const SisrConvDesc *d);
/* bf16 build: the generator's last conv (model_generator.py:52-53: 3x3, 64 -> 3, bf16 NHWC in, NCHW fp32 out, prologue
 * NONE / ACT, epilogue NONE / TANH) runs on conv_toimage.hip (1x1 GEMM onto 27 (cout, tap) columns + col2im gather)
 * behind sisr_conv2d_bf16; tells whether a filled descriptor will. */
int sisr_conv2d_toimage_eligible(const SisrConvDesc *d);
/* ... and with fp32 NHWC tensors (fp32 parity build; exact fp32 MFMA) behind sisr_conv2d_f32 */
int sisr_conv2d_toimage_f32_eligible(const SisrConvDesc *d);
int sisr_wgrad_plan_bf16(SisrWgradDesc *d, int32_t max_pixel_blocks);
/* wgrad_deep.hip: 3x3, pad 1, stride 1 | 2, Cin % 64 == 0, Cout % 64 == 0, NHWC bf16 operands (x prologue NONE / ACT / AFFINE_ACT,
 * gradient prologue any of the one- or two-tensor forms).  Call after sisr_wgrad_plan_bf16 (slab layout and sizes are shared with
 * the generic kernel); on success deep.enabled = 1 and sisr_wgrad_bf16_slabs answers deep.n_pb.  target_wg: 0 = default. */
int sisr_wgrad_deep_plan(SisrWgradDesc *d, int32_t target_wg);
/* a fully filled descriptor (operands, modes, storage flags) will run on wgrad_deep.hip */
int sisr_wgrad_deep_eligible(const SisrWgradDesc *d);
/* Several wgrad_deep.hip layers in one launch (a flat grid; deep.batch_first_wg, filled by the caller = the workgroups of the members
 * in front, n_cib * n_cob * n_pb each): table_host = n fully filled, eligible descriptors of one stride, all
 * with or all without a two-tensor gradient prologue; table_dev = the same bytes in device memory.  Plan each member with its share
 * of the chip as target_wg (sisr_wgrad_deep_plan): the batch then walks 3-4 times as many tiles per workgroup behind the same fixed
 * costs and writes a third of the slabs.  Results per layer are those of sisr_conv2d_wgrad_bf16 on the same plan. */
int sisr_wgrad_deep_batch(const SisrWgradDesc *table_host, const SisrWgradDesc *table_dev, int32_t n, void *stream);
/* The same idea for the persistent trunk kernel (wgrad_trunk.hip: 3x3, 64 -> 64, bf16 NHWC, H % 8 == 0, W % 16 == 0): n fully filled
 * descriptors that sisr_wgrad_trunk_eligible accepts, Cout = 64, ONE gradient-prologue kind (BNBWD or BNACT_BWD); wgs_per_layer
 * workgroups -- and slabs: rows of each descriptor's `slab` -- serve every layer, grid = n * wgs_per_layer (choose 256 / n: each
 * workgroup then walks its share of ONE layer's tiles back to back).  The kernel reads its own view of the descriptors:
 * sisr_wgrad_trunk_batch_args fills n * sisr_wgrad_trunk_batch_arg_bytes() bytes of HOST memory, the caller copies them to the device
 * and passes that copy as args_dev.  Per-tile arithmetic is that of sisr_conv2d_wgrad_bf16; only the partition into slabs differs. */
int sisr_wgrad_trunk_batch_arg_bytes(void);
int sisr_wgrad_trunk_batch_args(const SisrWgradDesc *descs, int32_t n, void *args_host);
int sisr_wgrad_trunk_batch(const SisrWgradDesc *descs, const void *args_dev, int32_t n, int32_t wgs_per_layer, void *stream);
/* ... and for the fp32-tensor trunk kernel (wgrad_trunk_f32.hip; exact fp32 or, with mfma_split set on every member, the split
 * contraction): descriptors sisr_wgrad_trunk_f32_eligible accepts, Cout = 64, one gradient-prologue kind, one mfma_split setting */
int sisr_wgrad_trunk_f32_batch_arg_bytes(void);
int sisr_wgrad_trunk_f32_batch_args(const SisrWgradDesc *descs, int32_t n, void *args_host);
int sisr_wgrad_trunk_f32_batch(const SisrWgradDesc *descs, const void *args_dev, int32_t n, int32_t wgs_per_layer, void *stream);
int sisr_conv2d_wgrad_bf16(const SisrWgradDesc *d, void *stream);
/* The trunk geometry with bf16 NHWC operands (x prologue NONE / ACT / AFFINE_ACT, gradient prologue BNBWD /
 * BNACT_BWD) runs on the persistent kernel of wgrad_trunk.hip behind sisr_conv2d_wgrad_bf16: one slab per workgroup,
 * whatever the plan's n_slabs says.  sisr_wgrad_bf16_slabs(d) = slabs the launch of a fully filled descriptor writes
 * -- size `slab` (rows of slab_stride floats) and the reduction with it. */
int sisr_wgrad_trunk_eligible(const SisrWgradDesc *d);
int sisr_wgrad_bf16_slabs(const SisrWgradDesc *d);
/* The same for the fp32 parity build: the trunk geometry with fp32 NHWC operands and H % 4 == 0, W % 16 == 0 runs on the
 * persistent exact-fp32 kernel of wgrad_trunk_f32.hip behind sisr_conv2d_wgrad_f32 (one slab per workgroup). */
int sisr_wgrad_trunk_f32_eligible(const SisrWgradDesc *d);
int sisr_wgrad_f32_slabs(const SisrWgradDesc *d);
/* bf16 build: the weight gradient of the generator's first conv (9x9 over the 3-channel NCHW fp32 image, bf16 NHWC
 * output gradient with no / activation-backward prologue, H % 8 == 0, W % 32 == 0) runs on wgrad_thin.hip (bf16 MFMA)
 * behind sisr_conv2d_wgrad_f32; tells whether a filled descriptor will (sisr_wgrad_f32_slabs accounts for it). */
int sisr_wgrad_thin_eligible(const SisrWgradDesc *d);
/* bf16 build: the weight gradient of the generator's last conv (3x3, 64 -> 3; bf16 NHWC x with prologue NONE / ACT, the
 * NCHW fp32 image gradient itself -- prologue NONE / TANH_BWD -- as g1 / g2, H % 8 == 0, W % 32 == 0, descriptor planned
 * by sisr_wgrad_plan_bf16 for the gradient padded to 4 channels) runs on wgrad_toimage.hip behind sisr_conv2d_wgrad_bf16:
 * no 4-channel NHWC copy of the gradient is needed then; same slab layout (sisr_wgrad_bf16_slabs accounts for it). */
int sisr_wgrad_toimage_eligible(const SisrWgradDesc *d);
/* ... and with fp32 NHWC activations (fp32 parity build; exact fp32 MFMA, descriptor planned by sisr_wgrad_plan) behind
 * sisr_conv2d_wgrad_f32; sisr_wgrad_f32_slabs accounts for it */
int sisr_wgrad_toimage_f32_eligible(const SisrWgradDesc *d);
int sisr_conv2d_wgrad_f32(const SisrWgradDesc *d, void *stream);
/* out[i] = sum_s slab[s][i], i < elems (also used for the bias slabs) */
int sisr_slab_reduce_f32(const float *slab, float *out, int32_t n_slabs, int64_t elems, int64_t lead_bf16, void *stream);
/* n_jobs independent reductions (arrays of n_jobs entries each, HOST memory: the jobs travel in the kernel arguments, eight per
 * launch) -- the weight gradients of one backward pass are summed by one launch instead of one per layer.  Same arithmetic and
 * order per job as sisr_slab_reduce_f32: bit-identical results. */
int sisr_slab_reduce_multi(const void *const *slabs, void *const *outs, const int32_t *n_slabs, const int64_t *elems,
                           const int64_t *lead_bf16, int32_t n_jobs, void *stream);
/* lead_bf16: the first lead_bf16 elements of every row are stored as bf16 at the row's start (what the persistent bf16
 * weight-gradient kernel writes: sisr_wgrad_bf16_slab_lead(d)), the rest -- the bias partials -- as fp32 at their float offset; 0: fp32 rows */
int64_t sisr_wgrad_bf16_slab_lead(const SisrWgradDesc *d);

/* ---- the kernel family a fully filled descriptor goes to.  Each of the four dispatchers (sisr_conv2d_bf16 / _f32,
 * sisr_conv2d_wgrad_bf16 / _f32) has ONE route function that holds the ordered chain of the sisr_*_eligible calls above; the
 * dispatcher and the sizing entry points its callers allocate from (*_parts, *_bnb_parts, *_slabs, *_slab_lead) switch on that
 * route, so no buffer is sized for another kernel than the one that runs -- and a caller that must know the family (which launches
 * can be batched, which layer needs a padded copy of its gradient) asks the same function instead of rebuilding the chain.
 * The values are ABI.  A dispatcher only returns the routes its chain holds (DEEP: the two bf16 ones; THIN: the two fp32 ones).
 * HOST only, no HIP call; SISR_E_BADARG for a null pointer. */
enum SisrRoute {
    SISR_ROUTE_GENERIC = 0,   /* the dispatcher's own tiled kernel (conv_fwd / conv_bf16 / conv_wgrad / wgrad_bf16 .hip)  */
    SISR_ROUTE_DEEP = 1,      /* conv_deep.hip / wgrad_deep.hip                                                            */
    SISR_ROUTE_TOIMAGE = 2,   /* conv_toimage.hip / wgrad_toimage.hip: the generator's last conv (64 -> 3)                 */
    SISR_ROUTE_TRUNK = 3,     /* the persistent trunk kernels (conv_trunk / conv_trunk_f32 / wgrad_trunk / wgrad_trunk_f32) */
    SISR_ROUTE_THIN = 4       /* conv_thin.hip / wgrad_thin.hip: convs over the 3-channel image                            */
};
int32_t sisr_conv2d_bf16_route(const SisrConvDesc *d);
int32_t sisr_conv2d_f32_route(const SisrConvDesc *d);
int32_t sisr_wgrad_bf16_route(const SisrWgradDesc *d);
int32_t sisr_wgrad_f32_route(const SisrWgradDesc *d);

/* ---- weights: spectral norm power iteration + packing (legacy torch.nn.utils.spectral_norm
 *      hook, model_generator.py:3; model_discriminator.py:2), multi-tensor: one launch serves
 *      every convolution of a network.  The descriptor TABLE lives in device memory. ---------- */
/* One packed image of a weight.  Every image is the same gather under one tap map: element (out, in, r', s') holds forward tap
 * (R0y + Sy r', R0x + Sx s') of W_orig (times 1 / sigma), and zero where that tap lies outside the weight:
 *   (R0, S) = (0, +1)       the forward conv                                                 transposed = 0
 *             (K - 1, -1)   the stride-1 data gradient (a conv over dy with flipped taps)    transposed = 1
 *             (c_R0, -2)    one output-parity class c = (py, px) of a stride-2 convolution's data gradient, itself a stride-1 conv
 *                           over dy with KH x KW taps                                        transposed = 1
 * transposed = 0: out = packed cout (SisrWeightDesc.shuffle2), in = cin; 1: out = cin, in = packed cout.  Out / in channels beyond
 * the weight's are zero.  `format` names the storage order: */
enum {
    /* fp32 [chunk of CK in][r'][out, CoutPad][krow, KROWP], krow = s' * PS + (in - chunk * CK); the slots in >= CK of a tap, the krow
     * slots behind the taps and the rows out >= the channel count are zero.  extra != 0 (trunk geometry: Cin = Cout = 64, 3x3): also
     * write, right behind the image (SISR_WLDS_WORDS more 32-bit words), the weights in the persistent fp32-tensor conv kernel's LDS
     * order -- [out half][chunk][tap][out 32][32 + 4 words] -- so that its weight fill is a plain 16-byte copy.  1: fp32 values; 2:
     * split build -- words 0..15 of a row the RNE bf16 heads of in-channels (2m, 2m + 1), words 16..31 the bf16 of what the heads
     * leave; words 32..35 zero */
    SISR_WIMG_F32 = 0,
    /* bf16 images for the bf16-MFMA kernels: [chunk of CK = 32 in][out, CoutPad][tap * CK + (in - chunk * CK)], n_chunk = in-channels
     * / CK.  extra != 0 (trunk geometry: 64 in-channels, 3x3, CoutPad % 64 == 0): also write, right behind the image (same size
     * again), the image in the order the persistent trunk kernels load it -- [32-out block][tap][k slice j: 16 in-channels][lane =
     * kk * 32 + out] x 8 bf16 (in-channels (j >> 1) * 32 + (j & 1) * 16 + 8 kk ..) -- so that a wave's 16-byte loads are contiguous
     * (1 KB per instruction instead of 64 pieces 576 bytes apart: 1.1 us of every launch) */
    SISR_WIMG_BF16 = 1,
    /* conv_deep.hip images (3x3 weights, channels in 32s; written by sisr_weights_pack_deep): bf16 [chunk of 32 in][r'][out, CoutPad]
     * [extra * 32 + 8], element s' * 32 + (in - chunk * 32), n_chunk = in-channels / 32, CoutPad = the out-channel count; the taps
     * s' >= KW of a row and its 8 padding elements are zero.  extra = taps per row: KW, or 2 where the four classes of a stride-2
     * data gradient run as one launch and every class image is written in the KW = 2 row format.  SisrWeightDesc.wdp_scaled = 0
     * packs W_orig itself (the kernels then apply 1 / sigma in their epilogue: SisrConvDesc.epi_scale_p), 1 packs W_orig / sigma */
    SISR_WIMG_DEEP = 2
};
typedef struct SisrWeightImage {
    void   *dst;               /* NULL: not written                                             */
    int32_t format;            /* SISR_WIMG_*                                                   */
    int32_t transposed;        /* 0: out = packed cout, in = cin;  1: out = cin, in = packed cout */
    int32_t KH, KW;            /* taps of the image                                             */
    int32_t R0y, Sy, R0x, Sx;  /* image tap (r', s') = forward tap (R0y + Sy r', R0x + Sx s')   */
    int32_t CK, PS, KROWP, n_chunk, CoutPad;   /* the consumer's plan (SisrConvPlan); see the formats */
    int32_t extra;             /* F32: LDS-order copy mode 0/1/2; BF16: lane-order copy 0/1; DEEP: taps per row */
} SisrWeightImage;
#define SISR_WLDS_WORDS (2 * 2 * 9 * 32 * 36)
#define SISR_WEIGHT_IMAGES 5

typedef struct SisrWeightDesc {
    const float *w_orig;      /* OIHW [Cout][Cin][KH][KW]                                     */
    float *u, *v;             /* spectral-norm buffers (updated in place when training) or NULL */
    float *u_used, *v_used;   /* copies of the u/v that define sigma (for backward) or NULL   */
    float *sigma;             /* [2] out: sigma (1.0 when u == NULL), 1 / sigma                */
    float *sn_work;           /* power-iteration scratch, >= ceil(Cout/16)*Cin*KH*KW + Cout floats (u != NULL) */
    int32_t Cout, Cin, KH, KW;
    int32_t training;         /* run the power iteration                                      */
    int32_t shuffle2;         /* conv feeds PixelShuffle(2): pack couts in (i,j)-major order  */
    int32_t wdp_scaled;       /* SISR_WIMG_DEEP images hold W_orig / sigma instead of W_orig  */
    /* [0]: the forward conv; [1]: the stride-1 data gradient, or [1 + c]: parity class c = 2 py + px of a stride-2 one */
    SisrWeightImage img[SISR_WEIGHT_IMAGES];
} SisrWeightDesc;
/* bytes sisr_weights_pack / sisr_weights_pack_deep write at img->dst (the copy `extra` asks for included; dst itself is not read),
 * or a negative status for a record no kernel packs (host only) */
int64_t sisr_weight_image_bytes(const SisrWeightImage *img);

/* max_rows / max_cols: largest Cout and Cin*KH*KW over the table (the launch grids are sized from them) */
int sisr_weights_prepare(const SisrWeightDesc *table_dev, int32_t n, int32_t max_rows, int32_t max_cols,
                         void *stream);

/* sisr_weights_prepare = sisr_weights_sn (power iteration: u, v, sigma; sigma[1] = 1 / sigma) + sisr_weights_pack (every image but
 * the SISR_WIMG_DEEP ones).  sisr_weights_pack_deep writes the conv_deep.hip images (SISR_WIMG_DEEP, 3x3 weights) from one
 * coalesced read of each 32 x 32-channel tile; max_cout / max_cin: largest channel counts over the table.  A caller that keeps
 * un-normalised images (wdp_scaled = 0) across the forwards between two optimizer steps runs sisr_weights_sn alone. */
int sisr_weights_sn(const SisrWeightDesc *table_dev, int32_t n, int32_t max_rows, int32_t max_cols, void *stream);
int sisr_weights_pack(const SisrWeightDesc *table_dev, int32_t n, int32_t max_rows, int32_t max_cols, void *stream);
int sisr_weights_pack_deep(const SisrWeightDesc *table_dev, int32_t n, int32_t max_cout, int32_t max_cin, void *stream);

/* Weight-gradient epilogue: packed dW (sum of slabs) -> OIHW gradient of w_orig, through the
 * spectral-norm quotient: dW_orig = (G - <G, W> u v^T) / sigma  (autograd of W = W_orig/sigma with
 * sigma = u.(W_mat v), u and v constant; spectral_norm.py compute_weight). */
typedef struct SisrWeightGradDesc {
    const float *dwpk;        /* [chunk][r][krow][CoutPad] reduced packed gradient            */
    const float *w_orig, *u_used, *v_used, *sigma;   /* u_used == NULL: no spectral norm      */
    float *grad;              /* OIHW out                                                     */
    const float *dbias_pk;    /* [CoutPad] reduced packed bias gradient or NULL               */
    float *grad_bias;         /* [Cout] out (original channel order) or NULL                  */
    int32_t Cout, Cin, KH, KW, shuffle2;
    int32_t CK, PS, KROWP, n_chunk, CoutPad;
    int32_t layout;           /* 0: fp32 wgrad slabs [chunk][r][krow][co]; 1: bf16 wgrad slabs
                                 [chunk32][tap][ci][co]                                          */
} SisrWeightGradDesc;

/* parts = the largest tile count of the table, tiles of a weight = ceil(Cout/32) * ceil(Cin/C) * ceil(KH*KW/tg) with C = 32 for
 * layout 1 (bf16 slabs) and CK otherwise, tg = 32 / min(C, Cin) taps per tile, at least 1 and at most KH*KW;
 * dot_work: >= parts*n floats of scratch */
/* workgroups along grid.y (= dot_work entries) one weight needs; `parts` >= the maximum over the table (host only) */
int sisr_weights_grad_tiles(const SisrWeightGradDesc *w);
int sisr_weights_grad(const SisrWeightGradDesc *table_dev, int32_t n, float *dot_work, int32_t parts, void *stream);
/* the same for a table of 3x3 weights with Cin % 32 == 0, layout 1 and no PixelShuffle permutation: whole 32 x 32 x 9 tiles, one
 * read of the packed gradient, the spectral-norm rank-one term as an elementwise pass afterwards (the discriminator's 8 convs:
 * 166 -> ~25 us per backward).  dot_work: n * ceil(max_cout / 32) * (max_cin / 32) floats. */
int sisr_weights_grad_fast(const SisrWeightGradDesc *table_dev, int32_t n, float *dot_work, int32_t max_cout, int32_t max_cin,
                           void *stream);

/* ---- BatchNorm2d (training) pieces that are not fused into the convolutions ------------------
 * finalize: merge the per-tile (mean, M2) partials (Chan et al.), produce the fused apply
 * constants scale = gamma*invstd, shift = beta - mean*scale, update the running statistics
 * (momentum 0.1, unbiased variance) -- nn.BatchNorm2d, model_generator.py:11,14,40. */
int sisr_bn_finalize(const float *stat_part, const float *cnt_part, int32_t n_tiles, int32_t C,
                     const float *gamma, const float *beta, float *running_mean, float *running_var,
                     float momentum, float eps, float *scale, float *shift, float *save_mean,
                     float *save_invstd, void *stream);
/* eval mode: scale/shift from the running statistics */
int sisr_bn_eval_consts(const float *gamma, const float *beta, const float *running_mean,
                        const float *running_var, float eps, int32_t C, float *scale, float *shift,
                        void *stream);

/* backward reductions over N*H*W for one BatchNorm (+ the activation that follows it):
 *   g  = (act_mode ? (z>0 ? dy : slope*dy) : dy),  z = scale[c]*x + shift[c]
 *   sum_g[c] = sum g ; sum_gx[c] = sum g*xhat,  xhat = (x-mean[c])*invstd[c]
 *   sum_slope = sum over z<=0 of dy*z   (gradient of a shared PReLU slope)
 * then the constants of SISR_PRO_BNBWD / SISR_PRO_BNACT_BWD:
 *   qa = gamma*invstd ; qb = -gamma*invstd^2*mean(g*xhat) ; qd = -qa*mean(g) - qb*mean
 * and dgamma = sum_gx, dbeta = sum_g, dslope (if act). */
typedef struct SisrBnBwdDesc {
    const float *dy, *x;                   /* NHWC [P][C]                                    */
    const float *scale, *shift, *mean, *invstd, *gamma;
    float *work;                           /* [grid][2*C+1] partials                          */
    float *qa, *qb, *qd;                   /* out [C]                                         */
    float *dgamma, *dbeta, *dslope;        /* out [C],[C],[1] (dslope may be NULL)            */
    int64_t P; int32_t C;
    int32_t act_mode;
    const float *slope_p; float slope;     /* device scalar slope, or NULL: use `slope`       */
    int32_t grid;                          /* filled by sisr_bn_bwd_plan                      */
    int32_t dy_bf16, x_bf16;               /* storage type of dy and x (0: fp32, 1: bf16)     */
} SisrBnBwdDesc;
int sisr_bn_bwd_plan(SisrBnBwdDesc *d);
int sisr_bn_bwd(const SisrBnBwdDesc *d, void *stream);
/* second half only: `work` holds d->grid partial rows [2*C+1] written by a conv epilogue (SisrConvDesc.bnb_part) */
int sisr_bn_bwd_finalize(const SisrBnBwdDesc *d, void *stream);
/* the same launch also carries a slab reduction (sisr_slab_reduce_f32's arguments) in additional workgroups: the
 * finishing step of a BatchNorm backward (a few latency-bound workgroups) and the slab sum of the weight gradient
 * computed just before it (hundreds of bandwidth-bound ones) are independent and adjacent in the backward schedule of
 * a residual block (model_generator.py:16-19 differentiated), so one launch replaces two -- 33 fewer per step.  Both
 * results are bit-identical to the separate launches. */
int sisr_bn_bwd_finalize_slab(const SisrBnBwdDesc *d, const float *slab, float *out, int32_t n_slabs, int64_t elems,
                              int64_t lead_bf16, void *stream);

/* elementwise: y = f(x1) + (pa ? pa[c]*x2 + pd[c] : x2)   over NHWC [P][C];
 * f = lrelu(., slope1_p ? *slope1_p : slope1) -- the residual add of BasicBlock.forward (model_generator.py:19) and the
 * long skip (model_generator.py:93) with the BatchNorm apply fused.  x2 may be NULL (y = f(x1)). */
/* Elementwise entry points take a storage word `dt`: bit k set = the k-th tensor argument (in argument order,
 * inputs then output) is bf16 instead of fp32 (SISR_DT(a, b, c) below); arithmetic is fp32 either way. */
#define SISR_DT(a, b, c) ((a) | ((b) << 1) | ((c) << 2))
int sisr_eltwise_res_affine(const float *x1, const float *slope1_p, float slope1, const float *x2,
                            const float *pa, const float *pd, float *y, int64_t P, int32_t C, int32_t dt /* x1, x2, y */,
                            void *stream);
/* sum over all elements where pre<=0 of dy*pre  -> out[0]  (gradient of a PReLU slope that is
 * not followed by... BatchNorm-free sites: model_generator.py:34,48) ; work: [grid] floats */
int sisr_prelu_slope_grad(const float *dy, const float *pre, int64_t n, float *work, float *out,
                          int32_t dt /* dy, pre */, void *stream);
/* The whole backward of the generator's last conv (model_generator.py:52-53: 3x3, 64 -> 3, stride 1, pad 1, + Tanh) with fp32
 * tensors in ONE pass over the two big tensors (toimage_bwd.hip): the upscale stage's pre-activation `pre` is read once, the
 * gradient `g` wrt its activated value is written once, and the weight / bias gradient slabs and the PReLU-slope gradient of that
 * stage come out of the same tiles -- instead of sisr_conv2d_wgrad_f32 + sisr_conv2d_f32 (data gradient) + sisr_prelu_slope_grad:
 *   dyt     = dy * (1 - out^2)   (out: the saved tanh output; NULL: dyt = dy)
 *   g[p][ci] = sum_(co,ky,kx) W[co][ci][ky][kx] * dyt[co][p + (1 - ky, 1 - kx)]        zero outside the image
 *   slab / bias_slab: what the weight-gradient kernel of wgrad_toimage.hip writes for x = lrelu(pre, slope), the same slab count
 *   dslope[0] = sum_(pre <= 0) g * pre        (accumulated in double; dslope_part: one DOUBLE partial per workgroup, added in a
 *                                              fixed order by a one-workgroup finishing launch and rounded once to fp32)
 * `wpk` is the layer's packed fp32 FORWARD image [chunk][ky][cout][kx * w_PS + cl] (row length w_KROWP, w_CoutPad couts, chunks
 * of w_CK channels); CK .. slab_elems describe the slab as SisrWgradDesc's plan fields do.  sisr_toimage_bwd_f32_parts(d) =
 * workgroups of the launch = rows of `slab` (slab_stride floats each) = doubles of `dslope_part`.  Eligible: that geometry,
 * H % 8 == 0, W % 32 == 0, fp32 tensors (pre_bf16 = g_bf16 = 0), N * H * W * 256 < 2^31; SISR_TOIMAGE_BWD=0 (and SISR_THIN=0)
 * answer 0 and the caller keeps the three separate kernels. */
typedef struct SisrToImageBwdDesc {
    const float *pre;                        /* [N,H,W,64] NHWC                                               */
    const float *dy, *out;                   /* [N,3,H,W] NCHW image gradient, saved tanh output or NULL      */
    const float *wpk;
    const float *slope_p;                    /* device scalar slope (PReLU weight); NULL: slope               */
    float *g;                                /* [N,H,W,64] NHWC                                               */
    float *slab, *bias_slab;
    void *dslope_part;                       /* [parts] doubles, 8-byte aligned                               */
    float *dslope;
    int32_t N, H, W, Cin, Cout;
    int32_t KH, KW, stride, pad_y, pad_x;
    int32_t pre_bf16, g_bf16;                /* storage type of pre and g (0: fp32, 1: bf16 -- not eligible)  */
    int32_t w_CK, w_PS, w_KROWP, w_CoutPad;
    int32_t CK, PS, KROWP, n_chunk, CoutPad, slab_elems;
    float slope;
    int64_t slab_stride;
} SisrToImageBwdDesc;
int sisr_toimage_bwd_f32_eligible(const SisrToImageBwdDesc *d);
int sisr_toimage_bwd_f32_parts(const SisrToImageBwdDesc *d);
int sisr_toimage_bwd_f32(const SisrToImageBwdDesc *d, void *stream);
int sisr_toimage_bwd_desc_bytes(void);       /* sizeof(SisrToImageBwdDesc): a binding verifies its mirror with it */
/* y = a + b (same shape) */
int sisr_add(const float *a, const float *b, float *y, int64_t n, int32_t dt /* a, b, y */, void *stream);

/* ---- layout materialisation ------------------------------------------------------------------
 * NHWC [N][H][W][C] -> NCHW destination with row stride `dst_stride` floats per image (so a feature
 * map can be written straight into its slot of a concatenated [B, sum] feature vector), applying
 * y = lrelu(pa ? pa[c]*x + pd[c] : x, slope).  Used for D's flatten (model_discriminator.py:59),
 * MaskedVGG's taps (model_content_extractor.py:57-60) and forward_no_end (model_generator.py:86). */
int sisr_nhwc_to_nchw(const float *x, const float *pa, const float *pd, const float *slope_p,
                      float slope, float *y, int64_t dst_stride, int32_t N, int32_t H, int32_t W,
                      int32_t C, int32_t x_bf16, void *stream);
/* inverse gather: NCHW source (row stride src_stride per image) -> NHWC, y = x * (mask_pre ?
 * (lrelu'(mask_pre)) : 1) is NOT applied here: plain layout change. */
int sisr_nchw_to_nhwc(const float *x, int64_t src_stride, float *y, int32_t N, int32_t H, int32_t W,
                      int32_t C, int32_t y_bf16, void *stream);
/* NCHW gradient (C <= Cpad channels) -> NHWC [N][H][W][Cpad] with zero padding channels; out != NULL fuses the
 * tanh backward g = dy*(1 - out^2) of the generator's last layer (model_generator.py:54, nn.Tanh after the
 * final conv).  Feeds the bf16 weight gradient of that 3-channel conv. */
int sisr_nchw_grad_to_nhwc4(const float *dy, const float *out, float *g, int32_t N, int32_t C, int32_t H,
                            int32_t W, int32_t Cpad, void *stream);

/* ---- MaxPool2d(2,2) of the VGG19 stack (model_content_extractor.py:43; floors odd sizes), NHWC.
 * Pooling commutes with the (monotonic) ReLU in front of it, so the forward pools the RAW conv
 * output and the consumer applies ReLU lazily; the backward fuses MaxPool' and ReLU':
 *   dx[argmax of the 2x2 window] = (x[argmax] > 0) ? dy : 0, all other positions 0
 * (first maximum in row-major window order, like ATen). */
int sisr_maxpool2_fwd(const float *x, float *y, int32_t N, int32_t H, int32_t W, int32_t C, int32_t dt /* x, y */,
                      void *stream);
int sisr_maxpool2_relu_bwd(const float *dy, const float *x, float *dx, int32_t N, int32_t H, int32_t W,
                           int32_t C, int32_t dt /* dy, x, dx */, void *stream);
/* out = a + (ref > 0 ? b : 0)   (a may be NULL: out = masked b) -- merges a tap gradient into the
 * gradient of the ReLU it was taken behind (MaskedVGG's in-place-ReLU aliasing). */
int sisr_add_relu_masked(const float *a, const float *b, const float *ref, float *out, int64_t n,
                         int32_t dt /* a, b, ref, out */, void *stream);

/* ---- fully connected layers of D (nn.Linear, model_discriminator.py:47-53); weight-streaming,
 *      HBM-bound on W[Nout][K] (75-302 MB).  x operand: lrelu(x, in_slope) applied on load. ------ */
/* y[b][n] = act( sum_k lrelu(x[b][k]) * W[n][k] + bias[n] ),  epi: 0 none, 1 sigmoid; B <= 16 */
int sisr_fc_forward(const float *x, float in_slope, const float *W, const float *bias, float *y,
                    int32_t B, int32_t K, int32_t Nout, int32_t epi, void *stream);
/* dx[b][k] = sum_n dy[b][n] * W[n][k]; work: [splits][B][K] floats, splits = sisr_fc_dgrad_splits */
int sisr_fc_dgrad_splits(int32_t K, int32_t Nout);
int sisr_fc_dgrad(const float *dy, const float *W, float *dx, float *work, int32_t B, int32_t K,
                  int32_t Nout, void *stream);
/* dW[n][k] = sum_b dy[b][n] * lrelu(x[b][k], in_slope); db[n] = sum_b dy[b][n] */
int sisr_fc_wgrad(const float *dy, const float *x, float in_slope, float *dW, float *db, int32_t B,
                  int32_t K, int32_t Nout, void *stream);
/* The whole classifier head of D (model_discriminator.py:47-53: Linear(K, N) -> LeakyReLU -> Linear(N, 1) -> Sigmoid) on the
 * exact-fp32 matrix instruction (fc_head.hip), B <= 16, K % 16 == 0 (forward) / K % 64 == 0 (data gradient), N % 128 == 0:
 *   forward:  h1 [B][N] = x W1^T + b1 (pre-activation, kept for the backward), y [B] = sigmoid(lrelu(h1, slope) . W2 + b2);
 *             ws: sisr_fc_head_ws_floats(N) floats.  W2 == NULL: first layer only.
 *   backward: from g [B] = dL/dy: d1 [B][N] = dL/dh1, dW2 [N], db2 [1], db1 [N]  (everything that is not W1-sized);
 *   sisr_fc1_dgrad: dx [B][K] = d1 W1.   dW1 = d1^T x stays with sisr_fc_wgrad (an outer product: write-bound). */
int sisr_fc_head_ws_floats(int32_t N);
int sisr_fc_head_forward(const float *x, const float *W1, const float *b1, const float *W2, const float *b2, float slope,
                         float *h1, float *y, float *ws, int32_t B, int32_t K, int32_t N, void *stream);
int sisr_fc_head_backward(const float *g, const float *y, const float *h1, const float *W2, float slope, float *d1,
                          float *dW2, float *db2, float *db1, int32_t B, int32_t N, void *stream);
int sisr_fc1_dgrad(const float *d1, const float *W1, float *dx, int32_t B, int32_t K, int32_t N, void *stream);
/* dW[n][k] = scale * sum_b dy[b][n] * x[b][k] for MANY rows (B <= 256; K % 128 == 0, N % 64 == 0) on the exact-fp32 matrix instruction:
 * the data-parallel form of the classifier head's weight gradient -- ranks exchange the two rank-16 FACTORS (dy, x: N_ranks x 1.2-4.8 MB
 * through an all-gather) instead of all-reducing their 75-302 MB product, and every rank forms the mean itself (scale = 1 / ranks)
 * from all N_ranks x 16 rows: the same bits on every rank. */
int sisr_fc_wgrad_rows(const float *dy, const float *x, float scale, float *dW, int32_t B, int32_t K, int32_t N, void *stream);
/* elementwise helpers for the tiny FC activations: dy_pre = dy * act'(...) */
int sisr_act_bwd(const float *dy, const float *ref, float *out, int64_t n, int32_t kind, float slope,
                 void *stream);   /* kind 0: leaky (ref = pre-activation), 1: sigmoid (ref = output) */

/* ---- dataset transform ---------------------------------------------------------------------------
 * replaces, for a batch of decoded images, the per-image transform of config.py:225-231
 *   transforms.Compose([transforms.Resize(image_size_hr[1:]), transforms.ToTensor(), transforms.Normalize(.5, .5)])
 * i.e. PIL.Image.resize(BILINEAR) (Pillow's ImagingResample, 8 bits per channel: anti-aliased separable triangle filter,
 * 22-bit fixed-point coefficients, rounding to uint8 after each pass), uint8 -> float32 / 255, (t - mean) / std.
 * Integer arithmetic throughout the resize: bit-exact with Pillow.
 * sisr_resize_coeffs: HOST function; returns the taps per output index (ksize) and, with non-NULL tables, fills
 *   bounds[out_size][2] = (first input index, tap count) and kk[out_size][ksize] for one axis.  ksize > 64 (a down-scale
 *   above ~31x) is SISR_E_UNSUPPORTED in BOTH call modes, so the size query already refuses what the fill would.
 * sisr_resize_u8_normalize: src [N][H0][W0][C] uint8 -> dst [N][C][H][W] float32 with device copies of the two tables. */
int sisr_resize_coeffs(int32_t in_size, int32_t out_size, int32_t *bounds, int32_t *kk);
int sisr_resize_u8_normalize(const unsigned char *src, float *dst, int32_t N, int32_t H0, int32_t W0, int32_t C,
                             int32_t H, int32_t W, const int32_t *bx, const int32_t *kx, int32_t ksx,
                             const int32_t *by, const int32_t *ky, int32_t ksy, float mean, float stdv, void *stream);

/* ---- bicubic degradation, align_corners=True, A=-0.75, clamp to [-1,1]
 *      (utils.py:16-31: F.interpolate(..., 'bicubic', align_corners=True) + _crop_lr) -------- */
int sisr_bicubic_fwd(const float *x, float *y, int32_t NC, int32_t H, int32_t W, int32_t Ho,
                     int32_t Wo, int32_t clamp, void *stream);
/* dx = transpose of the interpolation applied to dy (masked by the clamp when y_clamped is given); gather form:
 * every input pixel sums the output gradients that read it in a fixed order -- deterministic, no atomics */
int sisr_bicubic_bwd(const float *dy, const float *y_clamped, float *dx, int32_t NC, int32_t H,
                     int32_t W, int32_t Ho, int32_t Wo, void *stream);

/* ---- device-resident patch source: the decoded dataset [M][H0][W0][C] uint8 lives in device memory and
 *      every batch is sampled from it there: image, crop window and flips / transposition per sample.  Random numbers:
 *      Philox4x32-10 (Salmon et al., SC'11) with key = (seed low, seed high) and counter = (t low, t high, b, rank) for step t,
 *      sample b of the batch and data-parallel rank `rank`.  From its four words r0..r3, with mulhi32(a, n) = (a * n) >> 32:
 *          index = mulhi32(r0, M)   y0 = mulhi32(r1, H0 - h + 1)   x0 = mulhi32(r2, W0 - w + 1)   ops = r3 & ops_mask
 *      (no rejection loop: a value's probability is off by at most range / 2^32).  ops bit 0: horizontal flip, bit 1: vertical
 *      flip, bit 2: transposition (h == w only), applied in that order.  order 0 = random (i.i.d. with replacement) as above;
 *      order 1 = sequential, the reference's sampler with drop_last: index = ((t mod nb) * world + rank) * B + b with
 *      nb = M / (B * world), offsets and ops still drawn.
 *      SISR_E_BADARG before any HIP call for null pointers, sizes < 1, a window larger than the image, rank outside [0, world),
 *      ops_mask outside [0, 7] or with bit 2 while h != w, an unknown order and sequential order with nb == 0. ------------- */
/* One workgroup: t = *step_dev; draws_dev[b] = { index, y0, x0, ops } for every b < B; *step_dev = t + 1 (an ordinary store by
 * one thread behind a barrier).  The count lives in device memory, so a captured launch advances on every replay. */
int sisr_patch_draw(int64_t *step_dev, uint64_t seed, int32_t rank, int32_t world, int32_t order, int32_t B, int32_t M,
                    int32_t H0, int32_t W0, int32_t h, int32_t w, int32_t ops_mask,
                    int32_t *draws_dev /* [B][4]: index, y0, x0, ops */, void *stream);
/* HOST: the same arithmetic (one __host__ __device__ function) for step t >= 0 into host memory; no GPU involved */
int sisr_patch_draws_host(int64_t t, uint64_t seed, int32_t rank, int32_t world, int32_t order, int32_t B, int32_t M,
                          int32_t H0, int32_t W0, int32_t h, int32_t w, int32_t ops_mask, int32_t *draws_host);
/* Sample b = data[index, y0 : y0 + h, x0 : x0 + w, :] after hflip, vflip, transposition as its row of draws_dev says.
 * dst_kind 0: [B][C][h][w] fp32, ((float)u8 / 255.0f - mean) / stdv (ToTensor + Normalize, the expressions of
 * sisr_resize_u8_normalize); dst_kind 1: [B][h][w][C] uint8 (that entry point's input layout).  1 <= C <= 4.  The kernel clamps
 * index, y0, x0 into range and ignores bit 2 while h != w, so no table can make it touch memory outside data / dst.  One
 * workgroup per 32 x 32 window tile and sample, staged through LDS so that global reads and writes are both coalesced for all
 * eight operations.  SISR_E_TOOBIG for B or h / 32 above 65535. */
int sisr_patch_gather(const unsigned char *data, int32_t M, int32_t H0, int32_t W0, int32_t C, const int32_t *draws_dev,
                      int32_t B, int32_t h, int32_t w, float mean, float stdv, void *dst, int32_t dst_kind, void *stream);

/* ---- the same source over images of MIXED sizes, and a shuffled epoch.  One uint8 buffer holds M images, image i as
 *      [H][W][C] row-interleaved bytes from byte `offset` on (any offset; gaps between images are allowed); the table of M
 *      records lives in device memory beside it.  The host validates a table once (patches.PackedImages); the kernels do not
 *      trust it: a byte outside the buffer is never loaded. */
typedef struct SisrImageRec {
    int64_t offset;            /* first byte of the image inside the buffer                     */
    int32_t H, W;
} SisrImageRec;
/* sisr_patch_draw / sisr_patch_draws_host with the offsets drawn inside the DRAWN image: the same four Philox words,
 *          index as the order says   y0 = mulhi32(r1, H_i - h + 1)   x0 = mulhi32(r2, W_i - w + 1)   ops = r3 & ops_mask
 *      with H_i, W_i from table[index]; table NULL: every image is H0 x W0 (with a table H0 and W0 are not read).  A NULL table or
 *      a table of equal sizes with order 0 or 1 gives sisr_patch_draw's table bit for bit.
 *      order 2 = permuted (these two entry points only, with or without a table): every image at most once per epoch, in a new
 *      random order each epoch.  nb = M / (B * world) batches per epoch (nb == 0: SISR_E_BADARG), epoch e = t / nb, position
 *      p = ((t mod nb) * world + rank) * B + b, index = sigma_e(p), where sigma_e is a bijection of [0, M) that depends on
 *      (seed, e) alone -- never on rank or b: the ranks of an epoch hold disjoint images; the M - nb * B * world images that
 *      sigma_e puts last sit the epoch out.  sigma_e is the swap-or-not shuffle (Hoang, Morris, Rogaway, CRYPTO 2012), 24 rounds,
 *      no cycle walking, any M; round r = 0 .. 23, with Philox keyed by the seed:
 *          K = mulhi32(philox(e low, e high, r, 0xFFFFFFFF)[0], M)      x' = (K + M - x) mod M
 *          if (philox(e low, e high, max(x, x'), 0xFFFFFFFE - r)[0] & 1)  x = x'
 *      (word 3 of a sample's counter is its rank < 2^31, so no counter is used twice).
 *      The host entry point also refuses a table with an image smaller than the window; the device one cannot see its table and
 *      gives such an image offset 0 (the gather then clamps). */
int sisr_patch_draw_table(int64_t *step_dev, uint64_t seed, int32_t rank, int32_t world, int32_t order, int32_t B, int32_t M,
                          int32_t H0, int32_t W0, const SisrImageRec *table_dev /* NULL: uniform H0 x W0 */, int32_t h, int32_t w,
                          int32_t ops_mask, int32_t *draws_dev, void *stream);
int sisr_patch_draws_table_host(int64_t t, uint64_t seed, int32_t rank, int32_t world, int32_t order, int32_t B, int32_t M,
                                int32_t H0, int32_t W0, const SisrImageRec *table_host /* may be NULL */, int32_t h, int32_t w,
                                int32_t ops_mask, int32_t *draws_host);
/* sisr_patch_gather with base address and row pitch from table_dev[index]: the same tiles, the same two destination kinds, the
 * same two fp32 expressions.  index is clamped into [0, M) and y0, x0 into the drawn image's own range; offsets are 64-bit; a
 * byte at an offset outside [0, data_bytes) is not loaded and reads as 0. */
int sisr_patch_gather_table(const unsigned char *data, int64_t data_bytes, const SisrImageRec *table_dev, int32_t M, int32_t C,
                            const int32_t *draws_dev, int32_t B, int32_t h, int32_t w, float mean, float stdv, void *dst,
                            int32_t dst_kind, void *stream);

/* ---- randomised blur + noise degradation: y = clamp(bicubic(x (*) k) + sigma_n z), per-sample k and sigma_n.
 *      x [N][C][H][W] fp32, 1 <= C <= 4; k [N][K][K] fp32, K odd in 1..21, R = (K - 1) / 2; y [N][C][h][w], any h, w >= 1.
 *        blur      b[n,c,y,x] = sum_{dy,dx in [-R,R]} k[n][dy+R][dx+R] x[n,c,clamp(y+dy,0,H-1),clamp(x+dx,0,W-1)]   (correlation,
 *                  replicate border; k is used as given, not renormalised)
 *        resample  r = bicubic(b) exactly as sisr_bicubic_fwd (align_corners, A = -0.75, scale (in-1)/(out-1), clamped taps)
 *        noise     y = r + sigma_n[n] z, then with `clamp` the clamp to [-1, 1]; a NULL sigma_n: no noise
 *      Random numbers: Philox4x32-10 keyed by the seed as the patch source's, word 3 of the counter tagged (patch-source counters
 *      carry ranks < 2^31 or tags >= 0xFFFFFFE7 there).  u_i = ((r_i >> 8) + 0.5) 2^-24 in fp32.
 *        parameters of sample b at step t: counter {t low, t high, b, 0xFE010000 | rank}, 0 <= rank < 65536:
 *            sigma1 = lo + (hi - lo) u0   sigma2 = anisotropic ? lo + (hi - lo) u1 : sigma1   theta = pi u2   sigma_n = nlo + (nhi - nlo) u3
 *            weight(dy, dx) = exp(-(u^2 / sigma1^2 + v^2 / sigma2^2) / 2), u = cos(theta) dx + sin(theta) dy, v = -sin(theta) dx + cos(theta) dy,
 *            divided by the sum of the K^2 weights, added in fp32 in index order
 *        noise of output element e (flat index over [N][C][h][w]): group g = e / 4, counter {t low, t high, g, 0xFE020000 | rank}:
 *            z0, z1 = sqrt(-2 ln u0) (cos, sin)(2 pi u1), z2, z3 likewise from u2, u3; element e takes z[e mod 4]
 *            (logf / log1pf / cosf / sinf / sqrtf; ln u is taken from the exact 1 - u above 1/2).  N C h w >= 2^34: SISR_E_TOOBIG.
 *      Every entry point returns SISR_E_BADARG before any HIP call for null pointers, sizes < 1, K even or outside 1..21, C outside
 *      1..4, sigma lo > hi or lo <= 0, a negative noise bound or nlo > nhi, rank outside [0, 65536). ---------------------------------- */
/* One workgroup: t = *step_dev; kernels_dev [B][K][K], noise_sigma_dev [B], drawn_step_dev[0] = t; *step_dev = t + 1 (an ordinary
 * store by one thread behind a barrier: a captured launch advances on every replay). */
int sisr_degrade_draw(int64_t *step_dev, uint64_t seed, int32_t rank, int32_t B, int32_t K, float sigma_lo, float sigma_hi,
                      int32_t anisotropic, float noise_lo, float noise_hi, float *kernels_dev, float *noise_sigma_dev,
                      int64_t *drawn_step_dev, void *stream);
/* HOST: the same arithmetic (one __host__ __device__ text) for step t >= 0 into host memory, no GPU involved.  params_host (may be
 * NULL): [B][4] = sigma1, sigma2, theta, sigma_n. */
int sisr_degrade_params_host(int64_t t, uint64_t seed, int32_t rank, int32_t B, int32_t K, float sigma_lo, float sigma_hi,
                             int32_t anisotropic, float noise_lo, float noise_hi, float *kernels_host, float *noise_sigma_host,
                             float *params_host);
/* HOST: z of output elements first .. first + count - 1 at step t, no GPU involved */
int sisr_degrade_noise_host(int64_t t, uint64_t seed, int32_t rank, int64_t first, int64_t count, float *z_host);
/* One launch: one workgroup per tile of LR pixels and (n, c) stages the HR footprint in LDS (the sample's kernel arrives by
 * scalar loads), blurs the pixels the tile's taps read, resamples, adds the noise of step *step_dev (read only with a non-NULL noise_sigma) and clamps.
 * The tile shrinks with the HR / LR ratio so that the LDS stays under 64 KB; every ratio is served (a 1 x 1 tile always fits).
 * SISR_E_TOOBIG also for N C or the rows of tiles above 65535 (sisr_degrade_bwd: N C or H / 32 above 65535). */
int sisr_degrade_fwd(const float *x, const float *kernels, const float *noise_sigma /* [N] or NULL */, const int64_t *step_dev,
                     uint64_t seed, int32_t rank, float *y, int32_t N, int32_t C, int32_t H, int32_t W, int32_t K, int32_t h,
                     int32_t w, int32_t clamp, void *stream);
/* dx = B^T R^T (dy * m), m = [-1 < y_saved < 1] (NULL: m = 1); no gradient for the kernels or the noise.  Gather form, fixed
 * order, no atomics.  The transpose of the replicate border folds the padded coordinates onto the border pixel: row 0 collects
 * padded rows -R .. 0, row H - 1 rows H - 1 .. H - 1 + R, likewise in x; H or W below R is fine. */
int sisr_degrade_bwd(const float *dy, const float *y_saved, const float *kernels, float *dx, int32_t N, int32_t C, int32_t H,
                     int32_t W, int32_t K, int32_t h, int32_t w, void *stream);

/* ---- second-order degradation: a draw from seven kernel families with a noise row and a final sinc filter
 *      per sample, and the noise operator.  The blur and the resampling are sisr_degrade_fwd / sisr_degrade_bwd with these kernels.
 *      An event of probability p happens when u <= p (u in (0, 1]: p = 1 always, p = 0 never).  Draws of sample b at step t, from
 *      counters {t low, t high, b, tag | rank}, u_i as above:
 *        0xFE04  u0 blur on (blur_prob); off: the delta kernel, exactly 1 at the centre
 *                u1 k_eff = ksize_min + 2 min((int)(m u1), m - 1), m = (K - ksize_min) / 2 + 1: uniform over the odd sizes in
 *                   ksize_min .. K; weights outside the centred k_eff x k_eff square are exactly 0
 *                u2 family 6 = sinc (sinc_prob); u3 otherwise the first family i with kernel_probs[i] > 0 and
 *                   u3 <= kernel_probs[0] + .. + kernel_probs[i] (fp32, added in index order): 0 iso, 1 aniso, 2 generalized_iso,
 *                   3 generalized_aniso, 4 plateau_iso, 5 plateau_aniso
 *        0xFE05  sigma1 = lo + (hi - lo) u0   sigma2 likewise from u1   theta = pi u2   (iso forms and sinc: sigma2 = sigma1, theta = 0)
 *                beta = lo + (hi - lo) u3 in beta_g for families 2, 3, in beta_p for 4, 5; stored as 0 otherwise
 *        0xFE06  omega = lo + (pi - lo) u0, lo = pi / 3 for k_eff < 13 and pi / 5 otherwise (sinc; stored as 0 otherwise)
 *                u1 noise mode 1 = gaussian (gaussian_prob), else 2 = shot; 0 = none when noise_hi = shot_hi = 0
 *                u2 grey flag (grey_prob)   amplitude = lo + (hi - lo) u3 in the mode's range
 *        0xFE07  the final filter: u0 sinc (final_sinc_prob), else the delta kernel; u1 its k_eff, u2 its omega, as above
 *      Unnormalised weight at (dy, dx), with u, v of the Gaussian draw above and q = u^2 / sigma1^2 + v^2 / sigma2^2 (fp32):
 *        0, 1  exp(-q / 2)     2, 3  exp(-q^beta / 2)     4, 5  1 / (q^beta + 1)
 *        6     omega J1(omega r) / (2 pi r), r = sqrt(dx^2 + dy^2), and omega^2 / (4 pi) at the centre -- in double, J1 from its
 *              power series below 12 and Hankel's expansion above (1e-11), rounded to fp32; negative lobes are intended
 *      divided by the sum of the K^2 weights in the fixed order of the Gaussian draw (lane partial sums, then the butterfly).
 *      SISR_E_BADARG before any HIP call for null pointers (final_kernels may be NULL), B < 1, K even or outside 1..21, ksize_min
 *      even or outside 1..K, a probability outside [0, 1], kernel_probs not summing to 1 within 1e-6, a reversed range, sigma or
 *      beta lo <= 0, a negative noise bound, rank outside [0, 65536). ------------------------------------------------------------- */
typedef struct SisrDegradeMix {
    int32_t K, ksize_min;
    float blur_prob, sinc_prob;
    float kernel_probs[6];
    float sigma_lo, sigma_hi, beta_g_lo, beta_g_hi, beta_p_lo, beta_p_hi;
    float noise_lo, noise_hi, shot_lo, shot_hi;      /* amplitude ranges of the two noise modes */
    float gaussian_prob, grey_prob, final_sinc_prob;
} SisrDegradeMix;
int sisr_degrade_mix_bytes(void);                    /* sizeof(SisrDegradeMix), for the Python mirror */
/* One workgroup, the pattern of sisr_degrade_draw: t = *step_dev, *step_dev = t + 1, drawn_step_dev[0] = t.  kernels_dev [B][K][K],
 * final_kernels_dev [B][K][K] or NULL, params_dev [B][8] = family, k_eff, sigma1, sigma2, theta, beta, omega, blur flag,
 * noise_table_dev [B][4] = mode, grey flag, amplitude, 0. */
int sisr_degrade_draw_mix(int64_t *step_dev, uint64_t seed, int32_t rank, int32_t B, const SisrDegradeMix *mix, float *kernels_dev,
                          float *final_kernels_dev, float *params_dev, float *noise_table_dev, int64_t *drawn_step_dev, void *stream);
/* HOST: the same text for step t >= 0 into host memory, no GPU involved. */
int sisr_degrade_mix_host(int64_t t, uint64_t seed, int32_t rank, int32_t B, const SisrDegradeMix *mix, float *kernels_host,
                          float *final_kernels_host, float *params_host, float *noise_table_host);
/* y = clamp ? clamp(x + n, -1, 1) : x + n over x [N][C][h][w], C in 1..4, with the sample's row of noise_table [N][4]:
 *   mode 0  n = 0      mode 1  n = a z      mode 2  n = (a / 8) sqrt(clip((v + 1) / 2, 0, 1)) z   (shot noise: the Gaussian
 *   approximation of Poisson noise at 256 levels with scale a, in [-1, 1] units)
 *   colour (grey flag 0): v the element, z of its flat index e, the stream of sisr_degrade_fwd (tag 0xFE02);
 *   grey: v the pixel's luma (C = 3: 0.299 R + 0.587 G + 0.114 B, otherwise the channel mean), ONE z per pixel from its flat index
 *   over [N][h][w] under tag 0xFE08, the same n in every channel.
 * The step is read from *step_dev.  One thread per pixel, grid-stride.  N C h w >= 2^34: SISR_E_TOOBIG. */
int sisr_degrade_noise_fwd(const float *x, const float *noise_table, const int64_t *step_dev, uint64_t seed, int32_t rank, float *y,
                           int32_t N, int32_t C, int32_t h, int32_t w, int32_t clamp, void *stream);
/* dx = dy [-1 < y_saved < 1] (NULL: dx = dy): n is a constant under autograd, for shot noise too. */
int sisr_degrade_noise_bwd(const float *dy, const float *y_saved, float *dx, int32_t N, int32_t C, int32_t h, int32_t w, void *stream);
/* HOST: z of pixels first .. first + count - 1 of the grey stream at step t, no GPU involved */
int sisr_degrade_noise_grey_host(int64_t t, uint64_t seed, int32_t rank, int64_t first, int64_t count, float *z_host);

/* ---- differentiable JPEG round trip: y = J(x), x and y [N][C][H][W] fp32, C in {1, 3}, any H, W >= 1;
 *      tables [N][2][64] fp32 (luma, chroma; row-major 8 x 8, entries > 0).  All arithmetic of the forward in fp32:
 *         1. p = (x + 1) 127.5 -- no rounding to 8 bits, no clamp of the input
 *         2. C = 3: JFIF YCbCr   Y = .299 R + .587 G + .114 B   Cb = -.168735892 R - .331264108 G + .5 B + 128
 *                                Cr = .5 R - .418687589 G - .081312411 B + 128;      C = 1: the plane is Y
 *         3. pad on the right and at the bottom by edge replication to a multiple of the MCU: 8 x 8 pixels for SISR_JPEG_444 and
 *            for C = 1, 16 x 16 for SISR_JPEG_420
 *         4. SISR_JPEG_420: each chroma plane becomes the mean of its 2 x 2 pixels
 *         5. per 8 x 8 block: subtract 128, c = D b D^T with the orthonormal DCT-II matrix D[k][n] = a_k cos((2n + 1) k pi / 16)
 *         6. u = c / T with the sample's table (luma: tables[n][0], chroma: tables[n][1]), c^ = rintf(u) T
 *         7. b^ = D^T c^ D, add 128; SISR_JPEG_420: every chroma value is replicated 2 x 2
 *         8. R = Y + 1.402 (Cr - 128)   G = Y - .344136286 (Cb - 128) - .714136286 (Cr - 128)   B = Y + 1.772 (Cb - 128)
 *            (the inverse of the matrix of step 2, written out to fp32)
 *         9. with `clamp`: clamp to [0, 255];  crop to H x W;  y = p^ / 127.5 - 1
 *      (the +128 of Cb / Cr and the -128 of step 5 cancel and are not executed).
 *      Tables: libjpeg's, in integer arithmetic, from an integer quality q in [1, 100]: s = q < 50 ? 5000 / q : 200 - 2 q,
 *      T[i] = clamp((base[i] s + 50) / 100, 1, 255), base = the two Annex K tables in row-major order.
 *      Quality of sample b at step t: Philox4x32-10 keyed by the seed, counter {t low, t high, b, 0xFE030000 | rank},
 *      u0 = ((r0 >> 8) + 0.5) 2^-24 in fp32 as above, q = min(qlo + (int)((qhi - qlo + 1) u0), qhi).
 *      Every entry point returns SISR_E_BADARG before any HIP call for null pointers, sizes < 1, C outside {1, 3}, quality bounds
 *      outside 1..100 or qlo > qhi, rank outside [0, 65536), unknown subsampling or grad codes; SISR_E_TOOBIG for N or Hp / 16
 *      above 65535. ------------------------------------------------------------------------------------------------------------ */
enum { SISR_JPEG_444 = 0, SISR_JPEG_420 = 1 };              /* subsampling (420 with C = 1 is 444) */
enum { SISR_JPEG_GRAD_STE = 0, SISR_JPEG_GRAD_CUBIC = 1 };  /* surrogate derivative of the rounding */
/* One workgroup: t = *drawn_step_dev is READ and not advanced (the launch shares the step sisr_degrade_draw stored there);
 * quality_dev [B] int32, tables_dev [B][2][64]. */
int sisr_jpeg_tables(const int64_t *drawn_step_dev, uint64_t seed, int32_t rank, int32_t B, int32_t qlo, int32_t qhi,
                     int32_t *quality_dev, float *tables_dev, void *stream);
/* HOST: the same arithmetic (one __host__ __device__ text) for step t >= 0 into host memory, no GPU involved. */
int sisr_jpeg_tables_host(int64_t t, uint64_t seed, int32_t rank, int32_t B, int32_t qlo, int32_t qhi, int32_t *quality_host,
                          float *tables_host);
/* One launch: one workgroup per 16 x 64 pixel tile and sample; all planes of the tile pass through LDS, nothing intermediate
 * touches HBM. */
int sisr_jpeg_fwd(const float *x, const float *tables, float *y, int32_t N, int32_t C, int32_t H, int32_t W, int32_t subsampling,
                  int32_t clamp, void *stream);
/* dx = J^T dy: every linear stage transposed (the pad's transpose folds the padded rows / columns onto row H - 1 / column W - 1),
 * the clamp's mask [-1 < y_saved < 1] (NULL: no mask), the rounding's surrogate derivative s(u) per coefficient: SISR_JPEG_GRAD_STE
 * s = 1; SISR_JPEG_GRAD_CUBIC s = 3 (u - rint u)^2 with u recomputed from x_saved and tables (both may be NULL under STE) in DOUBLE
 * (u - rint u cancels: fp32 leaves s to 1e-4; s is continuous across a tie, so the forward's fp32 decisions do not matter).  No
 * gradient for the tables.  Gather form, fixed order, no atomics. */
int sisr_jpeg_bwd(const float *dy, const float *y_saved, const float *x_saved, const float *tables, float *dx, int32_t N, int32_t C,
                  int32_t H, int32_t W, int32_t subsampling, int32_t grad, void *stream);

/* ---- whole-image super-resolution in tiles: an image of any size is cut into overlapping windows of one
 *      shape, the generator runs over them as a batch and the SR tiles are stitched.  The table rows are sisr_patch_gather's
 *      (index, y0, x0, ops); tiles are numbered row-major over the outer product of the two axis plans. ------------------------- */
/* HOST, no HIP call: the plan of one axis of extent L (LR pixels) for windows of extent T with `halo` pixels of context on every
 * interior side.  L <= T: one window [0, L).  Otherwise core = T - 2 halo >= 1 (else SISR_E_BADARG), n = ceil((L - 2 halo) / core),
 * origins a_i = min(i core, L - T) (strictly increasing; a window that reaches a border is flush with it) and ownership boundaries
 * b_i = (a_{i+1} + a_i + T) / 2 for i < n - 1, b_{n-1} = L: window i owns [b_{i-1}, b_i) with b_{-1} = 0, and every owned pixel is
 * at least `halo` away from each window edge that is not an image border.  Returns n; a_out / b_out (`cap` entries each) may both
 * be NULL for the count alone; n > cap: SISR_E_TOOBIG.  SISR_E_BADARG for L < 1, T < 1, halo < 0, one NULL array, cap < 1. */
int sisr_tile_axis(int32_t L, int32_t T, int32_t halo, int32_t *a_out, int32_t *b_out, int32_t cap);
/* sisr_patch_gather for ONE fp32 source: tile b = src[:, y0 : y0 + th, x0 : x0 + tw] (src [C][H][W], already normalised) after
 * hflip, vflip, transposition as row b of table_dev says -> dst [n][C][th][tw], bit-copied.  Same clamping: y0, x0 into range, bit 2
 * ignored while th != tw, the index ignored; nothing outside src is read.  SISR_E_BADARG before any HIP call for null pointers,
 * sizes < 1, a window larger than the image, C outside 1..4; SISR_E_TOOBIG for n or th / 32 above 65535. */
int sisr_tile_gather_f32(const float *src, int32_t C, int32_t H, int32_t W, const int32_t *table_dev, int32_t n, int32_t th,
                         int32_t tw, float *dst, void *stream);
/* tiles: [E ny nx][C][scale th][scale tw] fp32, member e of the self-ensemble at rows e ny nx ... with the ops of its table rows
 * (the planner writes ops = e); ay / by, ax / bx: the two axis plans in DEVICE memory.  dst_kind 0: [C][scale H][scale W] fp32;
 * 1: [scale H][scale W][C] uint8.  Output pixel (Y, X), per axis at LR position p = (Y + 0.5) / scale and feather f:
 *     r_i = clamp(min(dL, dR), 0, 1)   dL = (p - (b_{i-1} - f)) / 2f (first tile: +inf)   dR = ((b_i + f) - p) / 2f (last: +inf)
 *     w_i = r_i / sum_j r_j            (f = 0: r_i is the indicator of the owned interval)
 * the 2-D weight is the product of the two axes'; 0 <= f <= halo keeps a weight's support inside its window.
 *     v_e = sum over the tiles with weight, ascending, of w * tile[inverse ops (Y - scale a_y, X - scale a_x)]
 *     v   = (sum_e v_e) (1 / E), e ascending; f = 0 and E = 1: the owning tile's value, copied
 * (the inverse of "hflip, vflip, transposition" is "transposition, vflip, hflip").  fp32: v.  uint8: p = (v stdv + mean) 255 in
 * fp32, q = floor(p + 0.5) clamped to [0, 255], NaN -> 0.  One launch, no atomics, plain vector stores: deterministic, capturable.
 * Origins are clamped into the image and tile coordinates into the tile: no table can make the kernel touch memory outside
 * tiles / dst.  SISR_E_BADARG before any HIP call for null pointers, sizes < 1, th > H or tw > W, scale not in {1, 2, 4, 8}, E not
 * in {1, 8}, E = 8 with th != tw, C outside 1..4, f outside [0, halo] (NaN included), an unknown dst_kind. */
int sisr_tile_stitch(const float *tiles, const int32_t *table_dev, const int32_t *ay_dev, const int32_t *by_dev, int32_t ny,
                     const int32_t *ax_dev, const int32_t *bx_dev, int32_t nx, int32_t C, int32_t H, int32_t W, int32_t th,
                     int32_t tw, int32_t scale, int32_t halo, float feather, int32_t E, float mean, float stdv, void *dst,
                     int32_t dst_kind, void *stream);

/* ---- image-quality metrics: per-image PSNR and SSIM of two NCHW fp32 batches (the reference reports neither: its to-do list,
 *      README.md:88).  View applied on load: `crop` pixels stripped from every side; C == 3 with luma != 0: the BT.601 full-range
 *      plane Y = 0.299 R + 0.587 G + 0.114 B instead of the three planes.  PSNR = 10 log10(data_range^2 / mse), +inf for equal
 *      images; SSIM: 11 x 11 Gaussian window (sigma 1.5), "valid" positions only, C1 = (0.01 data_range)^2, C2 = (0.03 data_range)^2,
 *      mean over planes and positions.  Two launches (tiles -> `work`, then a fixed-order sum in double), no atomics: bit-identical
 *      from call to call, nothing synchronises with the host. ---------------------------------- */
/* HOST: floats of workspace for the shapes below; < 0 (SISR_E_UNSUPPORTED / bad argument) when C is not 1 or 3,
 * crop < 0, or H - 2*crop < 11 or W - 2*crop < 11 */
int sisr_image_metrics_ws_floats(int32_t N, int32_t C, int32_t H, int32_t W, int32_t crop, int32_t luma);
/* a, b: [N][C][H][W] fp32; psnr / ssim: [N] fp32, either may be NULL (then not computed) */
int sisr_image_metrics(const float *a, const float *b, int32_t N, int32_t C, int32_t H, int32_t W,
                       int32_t crop, int32_t luma, float data_range, float *work,
                       float *psnr, float *ssim, void *stream);

/* ---- losses: the feature MSE of train.py:183-186 and the BCE of config.py:107, forward and backward, fp32.
 *      Fixed-order sums, no atomics: bit-identical from call to call; nothing synchronises with the host.  The upstream gradient
 *      `g` of the backward entry points is ONE float in DEVICE memory (it is never fetched).  Tensors need only 4-byte alignment:
 *      16-byte accesses are used when every pointer of a call sits at the same offset inside its 16-byte line. --------------- */
/* HOST: floats of workspace for a feature MSE over n elements; < 0 for n < 1 (bad argument) or n > 2^40 (too big) */
int sisr_mse_ws_floats(int64_t n);
/* loss[0] = weight * mean((a - b)^2) over n contiguous elements.  Two launches: one partial per workgroup of a capped grid
 * (2048, or SISR_PERSIST_MAX_WG) into `work`, then one workgroup adds them in double */
int sisr_mse_fwd(const float *a, const float *b, int64_t n, float weight, float *work, float *loss, void *stream);
/* db = c (b - a), da = -db with c = 2 weight g[0] / n; da / db: [n], either may be NULL (then not written).  One launch */
int sisr_mse_bwd(const float *a, const float *b, const float *g, int64_t n, float weight, float *da, float *db,
                 void *stream);
/* loss[0] = weight * mean_i -(t_i max(log p_i, -100) + (1 - t_i) max(log(1 - p_i), -100)), mean_p[0] = mean_i p_i; either may
 * be NULL.  t_vec: [n] targets, or NULL for the one target t_scalar.  One workgroup, any n >= 1.  No range check on p: a NaN
 * or an out-of-range element gives a NaN loss */
int sisr_bce_fwd(const float *p, const float *t_vec, float t_scalar, int64_t n, float weight, float *loss,
                 float *mean_p, void *stream);
/* dp_i = weight g[0] (p_i - t_i) / max(p_i (1 - p_i), 1e-12) / n (torch's formula and epsilon) */
int sisr_bce_bwd(const float *p, const float *t_vec, float t_scalar, int64_t n, float weight, const float *g,
                 float *dp, void *stream);

/* ---- image-space loss: structural + pixel term of two NCHW fp32 batches, forward and backward.  The view
 *      is the metrics' (crop, then luma for C == 3) and so is the SSIM; every term lives on the view:
 *          loss[n] = w_ssim (1 - SSIM[n]) + w_pix mean_{C',H',W'} rho(a - b)
 *          rho(d) = |d| (L1), sqrt(d^2 + eps^2) (Charbonnier), d^2 (MSE)
 *      Fixed-order sums, no atomics, plain vector stores: bit-identical from call to call; nothing synchronises with the host.
 *      The forward saves nothing: the backward recomputes the window moments from a and b.  SISR_E_UNSUPPORTED for C not in
 *      {1, 3}; SISR_E_BADARG before any HIP call for N < 1, crop < 0, a view smaller than 11 x 11 with SSIM on (1 x 1 without),
 *      a non-positive data_range, a negative eps, an unknown pix_kind, null pointers. ------------------------------------- */
enum { SISR_PIX_L1 = 0, SISR_PIX_CHARBONNIER = 1, SISR_PIX_MSE = 2 };
/* HOST: floats of workspace of the forward.  with_ssim != 0: one partial per 16 x 32 tile of window positions (the metrics' grid);
 * with_ssim == 0: per 16 x 32 tile of view pixels */
int sisr_image_loss_ws_floats(int32_t N, int32_t C, int32_t H, int32_t W, int32_t crop, int32_t luma, int32_t with_ssim);
/* loss: [N]; ssim / pix: [N] or NULL: SSIM[n] and the mean of rho.  The SSIM passes run when w_ssim != 0 or ssim != NULL, and
 * `work` is sized by the query with that with_ssim.  Two launches: tiles -> `work`, then per image a fixed-order sum in double */
int sisr_image_loss_fwd(const float *a, const float *b, int32_t N, int32_t C, int32_t H, int32_t W, int32_t crop, int32_t luma,
                        float data_range, float w_ssim, float w_pix, int32_t pix_kind, float eps, float *work, float *loss,
                        float *ssim, float *pix, void *stream);
/* da / db: [N][C][H][W], either may be NULL (then not computed); g: [N] upstream gradients in DEVICE memory.  Every element is
 * written: pixels of the cropped border get 0.  rho'(0) = 0 for L1.  The SSIM passes run when w_ssim != 0.  One launch */
int sisr_image_loss_bwd(const float *a, const float *b, const float *g, int32_t N, int32_t C, int32_t H, int32_t W, int32_t crop,
                        int32_t luma, float data_range, float w_ssim, float w_pix, int32_t pix_kind, float eps, float *da,
                        float *db, void *stream);

/* ---- multi-scale SSIM of two NCHW fp32 batches, forward and backward.  The view is the metrics' (crop, then
 *      luma for C == 3), applied once at the finest scale; level j + 1 is the 2 x 2 mean (stride 2, no padding: an odd last row /
 *      column is dropped) of level j; window, "valid" positions, C1 and C2 are the metrics' at every level.  With M = levels and
 *      cs = (2 s_ab + C2) / (s_a^2 + s_b^2 + C2), l = (2 mu_a mu_b + C1) / (mu_a^2 + mu_b^2 + C1) per window position:
 *          t_j[n,p] = mean of cs (j < M - 1), mean of l cs (j = M - 1);   MS[n,p] = prod_j t_j^{w_j}, exactly 0 when a t_j <= 0;
 *          ms[n] = mean_p MS[n,p]
 *      Fixed-order sums, no atomics, plain vector stores: bit-identical from call to call; nothing synchronises with the host.
 *      `weights`: HOST array of 5 floats, the first `levels` are used as given.  SISR_E_UNSUPPORTED for C not in {1, 3};
 *      SISR_E_BADARG before any HIP call for N < 1, crop < 0, levels outside 1..5, a level smaller than 11 x 11 (the view needs
 *      11 << (levels - 1) pixels a side), a data_range or a weight that is not positive and finite, null pointers;
 *      SISR_E_TOOBIG past INT32_MAX floats or workgroups. --------------------------------------------------------------------- */
/* HOST: floats of which = 0: one pyramid buffer (levels >= 1 of ONE input, [N][C'][H_j][W_j] each, level 1 first; 0 for one
 * level); 1: the forward's partials (one pair per 16 x 32 tile of window positions, all levels); 2: the backward's gradient planes
 * (two pyramid buffers: a's, then b's) */
int sisr_ms_ssim_ws_floats(int32_t N, int32_t C, int32_t H, int32_t W, int32_t crop, int32_t luma, int32_t levels, int32_t which);
/* pyr_a / pyr_b: pyramid buffers, written (may be NULL for one level); part: the partials; terms: [levels][N][C'] = t_j[n,p];
 * ms: [N].  levels + 1 launches: one tile kernel per level (it also writes the next level), then per image a fixed-order sum in
 * double */
int sisr_ms_ssim_fwd(const float *a, const float *b, int32_t N, int32_t C, int32_t H, int32_t W, int32_t crop, int32_t luma,
                     float data_range, int32_t levels, const float *weights, float *pyr_a, float *pyr_b, float *part,
                     float *terms, float *ms, void *stream);
/* the gradient of sum_n g[n] (1 - ms[n]).  pyr_a / pyr_b / terms: as the forward left them; g: [N] upstream gradients in DEVICE
 * memory; work: the gradient planes (may be NULL for one level); da / db: [N][C][H][W], either may be NULL (then not computed).
 * Every element is written: pixels of the cropped border get 0, and so does every pixel of an (image, plane) with a term <= 0.
 * `levels` launches, coarsest level first */
int sisr_ms_ssim_bwd(const float *a, const float *b, const float *pyr_a, const float *pyr_b, const float *terms, const float *g,
                     int32_t N, int32_t C, int32_t H, int32_t W, int32_t crop, int32_t luma, float data_range, int32_t levels,
                     const float *weights, float *work, float *da, float *db, void *stream);

/* ---- frequency-domain loss of two NCHW fp32 batches, forward and backward.  The view is the metrics'
 *      (crop, then luma for C == 3): [N][C'][H'][W'].  With d = view(a) - view(b), D[kh, kw] = sum_{y,x} d[y, x]
 *      exp(-2 pi i (kh y / H' + kw x / W')) and Wh = W' / 2 + 1:
 *          L1, Charbonnier: loss[n] = mean over (C', kh < H', kw < Wh, {Re, Im}) of rho(.), rho(z) = |z|, sqrt(z^2 + eps^2)
 *                           (the half spectrum as rfft2 returns it, unnormalised, no Hermitian doubling; rho'(0) = 0 for L1)
 *          focal:           loss[n] = sum_p sum_{kh, kw < Wh} h |D|^(2 + alpha) / (max_p |D|^alpha (H' W')^2 C'), h = 1 for kw = 0 and
 *                           (W' even) kw = W' / 2, otherwise 2: the focal frequency loss over the full ortho-normalised spectrum with
 *                           the weight matrix |D|^alpha / max |D|^alpha per (n, plane) held constant for the gradient; a plane with
 *                           a == b has loss 0 and gradient 0
 *      A direct separable DFT with the twiddle tables in LDS: any view side 1 .. SISR_FREQ_MAX_SIDE.  Fixed-order sums, no atomics,
 *      plain vector stores: bit-identical from call to call; nothing synchronises with the host.  SISR_E_UNSUPPORTED for C not in
 *      {1, 3}; SISR_E_BADARG before any HIP call for N < 1, crop < 0, a view side outside 1 .. SISR_FREQ_MAX_SIDE, a negative eps,
 *      alpha outside (0, 4], an unknown kind, null pointers; SISR_E_TOOBIG past INT32_MAX floats or workgroups. ------------------- */
enum { SISR_FREQ_L1 = 0, SISR_FREQ_CHARBONNIER = 1, SISR_FREQ_FOCAL = 2 };
#define SISR_FREQ_MAX_SIDE 256
/* HOST: floats of which = 0: the forward's `work` (the row spectra [N][C'][H'][Wh][2], then one (sum, max) pair per workgroup of the
 * column pass); 1: `spec`, the saved spectrum [N][C'][H'][Wh][2]; 2: `pmax`, the plane maxima [N][C']; 3: the backward's `work` */
int sisr_freq_loss_ws_floats(int32_t N, int32_t C, int32_t H, int32_t W, int32_t crop, int32_t luma, int32_t which);
/* loss: [N].  spec: D itself, written when not NULL (all the backward needs: the inputs are not read again).  pmax: max |D|^2 per
 * (n, plane), written for focal (not NULL then), untouched otherwise.  eps is read for Charbonnier, alpha for focal; both are
 * checked for every kind.  Three launches: rows, columns + partial sums, then per image a fixed-order sum in double */
int sisr_freq_loss_fwd(const float *a, const float *b, int32_t N, int32_t C, int32_t H, int32_t W, int32_t crop, int32_t luma,
                       int32_t kind, float eps, float alpha, float *work, float *spec, float *pmax, float *loss, void *stream);
/* spec / pmax: as the forward left them; g: [N] upstream gradients in DEVICE memory; da / db: [N][C][H][W], either may be NULL
 * (then not computed; db is -da bit for bit).  Every element is written: pixels of the cropped border get 0.  Two launches */
int sisr_freq_loss_bwd(const float *spec, const float *pmax, const float *g, int32_t N, int32_t C, int32_t H, int32_t W,
                       int32_t crop, int32_t luma, int32_t kind, float eps, float alpha, float *work, float *da, float *db,
                       void *stream);

/* ---- separable Gaussian filter with a mirrored border, forward and backward, and the unsharp mask on it.
 *      Tensors are fp32 [N][C][H][W], contiguous; `planes` = N C.  K odd, 1 .. SISR_GAUSS_MAX_K, R = K / 2:
 *          y[i][j] = sum_{a, b} t[a] t[b] x[m(i + a - R)][m(j + b - R)],  m(p) = -p below 0, 2 (L - 1) - p from L on
 *      (torch's 'reflect', OpenCV's BORDER_REFLECT_101: the edge pixel is not repeated).  The mirror needs H > R and W > R: smaller
 *      planes return SISR_E_UNSUPPORTED.  SISR_E_BADARG before any HIP call for null pointers, K even or outside
 *      1 .. SISR_GAUSS_MAX_K, sizes < 1, an output whose bytes overlap an input's or another output's (checked on the byte ranges:
 *      the tiles read their neighbours' pixels), lo >= hi or settings that are not finite; SISR_E_TOOBIG for H W or the workgroup
 *      count (planes times the 32 x 64 tiles of a plane) above INT32_MAX.  One launch per filter, LDS only between the two passes,
 *      fixed summation order, no atomics, plain vector stores: the same bits on every call, and nothing is read back by the host.
 *      A non-finite input value reaches the outputs inside the filter's support and no others (a term outside it is 0 x 0, never 0 times
 *      the value). --------------------------------------------------------------------------------------------------------- */
#define SISR_GAUSS_MAX_K 63
/* HOST: t_i = exp(-(i - (K - 1) / 2)^2 / (2 sigma^2)) / sum, evaluated and normalised in double, rounded once.  sigma <= 0: OpenCV's
 * rule sigma = 0.3 ((K - 1) / 2 - 1) + 0.8 (8.0 at K = 51) -- with the FORMULA for every K: OpenCV's tabulated kernels for K <= 7 are
 * not reproduced.  taps_host: K floats of host memory */
int sisr_gauss_taps_host(int32_t K, float sigma, float *taps_host);
/* taps_dev: K floats in device memory (any K taps: nothing below assumes they are symmetric or sum to 1) */
int sisr_gauss_blur_fwd(const float *x, const float *taps_dev, float *y, int64_t planes, int32_t H, int32_t W, int32_t K,
                        void *stream);
/* dx = G^T dy, the exact transpose of the forward, in gather form */
int sisr_gauss_blur_bwd(const float *dy, const float *taps_dev, float *dx, int64_t planes, int32_t H, int32_t W, int32_t K,
                        void *stream);
/* HOST: bytes of the unsharp mask's workspace, one float and one byte per element; < 0: a status code */
int64_t sisr_usm_ws_bytes(int64_t planes, int32_t H, int32_t W);
/* Real-ESRGAN's USMSharp with s = 255 / (hi - lo):  blur = G x;  res = x - blur;  mask = |res| s > threshold (bytes 0 / 1);
 * soft = G mask;  sharp = min(max(x + weight res, lo), hi);  y = x + soft (sharp - x) -- that recipe's soft sharp + (1 - soft) x,
 * written so that weight = 0 or an all-zero mask returns x bit for bit.  Two launches: the first leaves blur and the mask in ws,
 * the second filters the mask and combines.  mask_out: [N][C][H][W] bytes, or NULL.  y, ws and mask_out share no byte with x, the
 * taps or each other (SISR_E_BADARG) */
int sisr_usm_fwd(const float *x, const float *taps_dev, int32_t K, float weight, float threshold, float lo, float hi, void *ws,
                 float *y, uint8_t *mask_out, int64_t planes, int32_t H, int32_t W, void *stream);

/* ---- artifact-aware (locally discriminative, LDL) image loss: the refined artifact map of Liang et al. (CVPR 2022) and the L1 it
 *      weighs, forward and backward.  sr, gt, ema: fp32 [N][C][H][W], contiguous, C 1 or 3; K = ksize odd,
 *      3 .. SISR_ARTIFACT_MAX_K, P = K / 2, H > P and W > P:
 *          r_sr[n,y,x] = sum_c |gt - sr|,   r_ema[n,y,x] = sum_c |gt - ema|
 *          p[n]        = Var(r_sr[n,:,:])^(1/5)                       (unbiased: divisor H W - 1)
 *          v[n,y,x]    = Var of r_sr[n] over the K x K window at (y, x) (unbiased: divisor K K - 1), coordinates outside the plane
 *                        mirrored without repeating the edge pixel: -q below 0, 2 (L - 1) - q from L on (the rule of sisr_gauss_*)
 *          map[n,y,x]  = p[n] v[n,y,x], exactly 0 where r_sr < r_ema  (strict: a tie keeps the weight)
 *          loss[n]     = weight mean_{c,y,x} map |sr - gt|            = weight sum_{y,x} map r_sr / (C H W)
 *      The map is a CONSTANT of the loss: dsr = g[n] weight map sign(sr - gt) / (C H W), dgt = -dsr, sign(0) = 0, nothing for ema.
 *      Both variances are taken around a value of the data (shifted sums in double, count / mean / M2 partials merged in a fixed
 *      order; the window's in two passes), never as a difference of raw moments.  Fixed-order sums, no atomics, plain vector stores:
 *      the same bits on every call, and nothing is read back by the host.  SISR_E_BADARG before any HIP call for null pointers, a
 *      workspace that is not 8-byte aligned, N < 1, H or W < 1, K even or outside 3 .. SISR_ARTIFACT_MAX_K, a weight that is not finite;
 *      SISR_E_UNSUPPORTED for C not in {1, 3} and for H <= P or W <= P; SISR_E_TOOBIG for N C H W or the workspace above INT32_MAX
 *      floats. ------------------------------------------------------------------------------------------------------------------ */
#define SISR_ARTIFACT_MAX_K 11
/* HOST: floats of the forward's workspace: the two residual planes [N][H][W], the (count, mean, M2) partials of every sample and
 * one partial sum per 8 x 64 tile, the last two kept as doubles; < 0: a status code */
int sisr_artifact_ws_floats(int32_t N, int32_t H, int32_t W);
/* map: [N][H][W]; loss: [N], or NULL for the map alone.  ws: 8-byte aligned.  Three launches (two without loss): the residual
 * planes and the samples' variance partials; an 8 x 64 tile of r_sr with its mirrored halo in LDS -> window variance, p[n] from the
 * merged partials, mask, map and the tile's sum of map r_sr; per sample a fixed-order sum in double */
int sisr_artifact_fwd(const float *sr, const float *gt, const float *ema, int32_t N, int32_t C, int32_t H, int32_t W, int32_t ksize,
                      float weight, void *ws, float *map, float *loss, void *stream);
/* map: as the forward left it; g: [N] upstream gradients in DEVICE memory; dsr / dgt: [N][C][H][W], either may be NULL (then not
 * written; dgt is -dsr bit for bit).  One elementwise launch */
int sisr_artifact_bwd(const float *sr, const float *gt, const float *map, const float *g, int32_t N, int32_t C, int32_t H, int32_t W,
                      float weight, float *dsr, float *dgt, void *stream);

/* ---- multi-tap perceptual loss with a Gram-matrix style term (BasicSR's PerceptualLoss), forward and backward.
 *      fa, fb: fp32 [B][total], contiguous: the output layout of MaskedVGG.forward.  shapes: HOST array [n_taps][3] of (C, H, W) with
 *      sum_l C_l H_l W_l == total; tap l is columns [off_l, off_l + C_l P_l) of every row in NCHW order, P_l = H_l W_l, F_x,l[n] that
 *      slice as C_l x P_l.  layer_w: HOST array [n_taps].  Per tap, with crit one of SISR_PERCEP_L1 (mean |d|), SISR_PERCEP_L2
 *      (mean d^2), SISR_PERCEP_FRO (sqrt(sum d^2) over the whole batch tensor of the tap):
 *          T_l = crit(fa_l, fb_l)      G_x,l[n] = F_x,l[n] F_x,l[n]^T / (C_l P_l)      S_l = crit(G_a,l, G_b,l) over its B C_l^2 elements
 *          perceptual = perceptual_weight sum_l w_l T_l          style = style_weight sum_l w_l S_l
 *      A term whose weight is 0 is not computed: none of its launches happen and its outputs are not written.  The Gram products run
 *      on v_mfma_f32_32x32x2_f32 (exact fp32 products), 32 x 32 tiles on or above the diagonal with the mirror stored from the same
 *      sums (G is bit-symmetric), P split across workgroups with the partials added in split order; every reduction over a tensor is
 *      a fixed-order sum in double.  No atomics, nothing read back by the host: the same bits on every call.  sign(0) = 0; a zero
 *      Frobenius norm gives an all-zero gradient; a NaN in gives NaN terms.  SISR_E_BADARG before any HIP call for null pointers, a
 *      workspace that is not 16-byte aligned, B < 1, n_taps outside 1 .. SISR_PERCEP_MAX_TAPS, a non-positive dim, a shape sum that is
 *      not total, an unknown criterion, both weights 0; SISR_E_TOOBIG for a tap of more than INT32_MAX elements per sample. ------- */
#define SISR_PERCEP_MAX_TAPS 8
#define SISR_PERCEP_L1 0
#define SISR_PERCEP_L2 1
#define SISR_PERCEP_FRO 2
/* HOST: bytes of the workspace, in this order: one double per workgroup of the feature pass (with_feature), one per workgroup of the
 * Gram finish and the [C][C] Gram partials of both inputs, samples and splits of P (with_style); < 0: a status code.  The Gram-only
 * entry takes the with_style size. */
int64_t sisr_percep_ws_bytes(int32_t B, int32_t n_taps, const int32_t *shapes, int32_t with_feature, int32_t with_style);
/* gram: the taps' G [B][C_l][C_l] one after the other (sum_l B C_l^2 floats), the bits the loss forms internally.  Two launches */
int sisr_percep_gram(const float *f, int32_t B, int64_t total, int32_t n_taps, const int32_t *shapes, void *ws, float *gram,
                     void *stream);
/* terms_p / terms_s: [n_taps] tables of T_l / S_l (either may be NULL); perceptual / style: the scalars, required when their weight
 * is not 0; dmat: NULL, or sum_l B C_l^2 floats that receive D_l[n] = dS_l / dG_a,l[n] for the backward (l1: sign(d) / (B C^2), l2:
 * 2 d / (B C^2), fro: d, the norm S_l dividing in the backward).  Launches: Gram partials, Gram finish (style), feature pass
 * (perceptual), tables and scalars: four with both terms, whatever B is */
int sisr_percep_fwd(const float *fa, const float *fb, int32_t B, int64_t total, int32_t n_taps, const int32_t *shapes,
                    const float *layer_w, float perceptual_weight, float style_weight, int32_t crit, void *ws, float *terms_p,
                    float *terms_s, float *perceptual, float *style, float *dmat, void *stream);
/* dmat, terms_p, terms_s: as the forward left them (the tables are read for SISR_PERCEP_FRO only); g_perceptual / g_style: the
 * upstream gradients of the two scalars in DEVICE memory, required when their weight is not 0; dfa / dfb: [B][total], either may be
 * NULL (then not computed).  dstyle / dF_a = (2 / (C P)) D F_a and dstyle / dF_b = -(2 / (C P)) D F_b on the same instruction with the
 * feature term's derivative added in the epilogue: one launch, every element stored exactly once */
int sisr_percep_bwd(const float *fa, const float *fb, const float *dmat, const float *terms_p, const float *terms_s,
                    const float *g_perceptual, const float *g_style, int32_t B, int64_t total, int32_t n_taps, const int32_t *shapes,
                    const float *layer_w, float perceptual_weight, float style_weight, int32_t crit, float *dfa, float *dfb,
                    void *stream);

/* ---- contextual loss (Mechrez, Talmi, Zelnik-Manor, ECCV 2018), cosine form, over the taps of a feature vector, forward and backward
 *      (DESIGN.md section 31).  fa (the generator side), fb (the target, a constant of the loss): fp32 [B][total], contiguous, taps and
 *      shapes as sisr_percep_fwd takes them; X[n], Y[n] the C x P slices of a tap, column i the feature point x_i.  Per tap:
 *          mu = the channel-wise mean of Y over batch and points      x^_i = (x_i - mu) / max(|x_i - mu|, 1e-12),  y^_j likewise
 *          S_ij = x^_i . y^_j    d_ij = 1 - S_ij    m_i = min_j d_ij    w_ij = exp((1 - d_ij / (m_i + 1e-5)) / band_width)
 *          Z_i = sum_j w_ij    CX_ij = w_ij / Z_i    c_j = max_i CX_ij    CX[n] = (1 / P) sum_j c_j
 *          T_l = (1 / B) sum_n -log(CX[n] + 1e-5)      loss = weight sum_l w_l T_l
 *      Ties of the min and of the max take the lowest index.  S runs on v_mfma_f32_32x32x2_f32 with K = C over the centred features, the
 *      two 1 / norm factors scale the 32 x 32 tile in the epilogue; mu, the squared norms, Z, CX[n] and the terms are summed in double in
 *      a fixed order.  No atomics, nothing read back by the host: the same bits on every call.  A NaN in gives a NaN term.
 *      SISR_E_BADARG before any HIP call for null pointers, tables that are not 4-byte or a workspace that is not 16-byte aligned, B < 1,
 *      n_taps outside 1 .. SISR_PERCEP_MAX_TAPS, a non-positive dim, a shape sum that is not total, a band_width that is not a finite
 *      positive number, an unknown `which`; SISR_E_TOOBIG for a tap of more than SISR_CX_MAX_POINTS points (take a deeper tap or pool the
 *      features). ------- */
#define SISR_CX_MAX_POINTS 2304
#define SISR_CX_WS_TABLES 0
#define SISR_CX_WS_SIM 1
#define SISR_CX_WS_FWD 2
#define SISR_CX_WS_BWD 3
/* HOST: bytes of TABLES: mu (sum_l C_l floats) and seven tables of B sum_l P_l elements, tap after tap as [B][P_l]: |x_i - mu|, |y_j - mu|,
 * m, Z, c (floats), j*, i* (int32) -- what the backward needs beside the inputs and CX[n]; SIM: the taps' S [B][P_l][P_l] one after the
 * other; FWD: one double per workgroup of the column pass, then S; BWD: S, then dloss / dx^ [B][total].  < 0: a status code */
int64_t sisr_cx_ws_bytes(int32_t B, int32_t n_taps, const int32_t *shapes, int32_t which);
/* sim: SIM floats, the bits the loss forms internally; tab: TABLES (mu and the two norm tables are written).  Three launches */
int sisr_cx_sim(const float *fa, const float *fb, int32_t B, int64_t total, int32_t n_taps, const int32_t *shapes, void *tab, float *sim,
                void *stream);
/* layer_w: HOST array [n_taps].  tab: TABLES, all written; ws: FWD; terms: [n_taps] T_l or NULL; cx: [n_taps][B] CX[n]; loss: the scalar.
 * Six launches, whatever B is */
int sisr_cx_fwd(const float *fa, const float *fb, int32_t B, int64_t total, int32_t n_taps, const int32_t *shapes, const float *layer_w,
                float band_width, float weight, void *tab, void *ws, float *terms, float *cx, float *loss, void *stream);
/* tab, cx: as the forward left them; g: the upstream gradient of the scalar in DEVICE memory; ws: BWD; dfa: [B][total], every element
 * stored once.  S is recomputed by the forward's kernel, a row pass turns it into -dloss / dd in place (r_i gathered from the i* table),
 * dloss / dx^ = Y^ T^T runs on the same instruction with K = P, a thin launch applies the normalisation's projection (0 where
 * |x_i - mu| < 1e-12).  Four launches.  There is no gradient for fb */
int sisr_cx_bwd(const float *fa, const float *fb, const void *tab, const float *cx, const float *g, int32_t B, int64_t total,
                int32_t n_taps, const int32_t *shapes, const float *layer_w, float band_width, float weight, void *ws, float *dfa,
                void *stream);

/* ---- image resize with torch's half-pixel coordinates, the mode chosen per sample, forward and backward.
 *      x [N][C][H][W] fp32, contiguous -> y [N][C][h][w], any h, w >= 1, up or down, any ratio.  modes [N] int32 in DEVICE memory, one
 *      per sample: the host never reads it, so a captured launch follows whatever the table holds at replay.  A value outside 0 .. 2
 *      is treated as SISR_RESIZE_BICUBIC (it indexes nothing).  y = R_h x R_w^T; row o of the 1-D operator R for `in` -> `out`, in integer
 *      arithmetic (64-bit; nothing depends on an fp32 scale):
 *        area      s = floor(o in / out), e = ceil((o + 1) in / out): weight 1 / (e - s) on s .. e - 1          (adaptive_avg_pool2d,
 *                  which is what F.interpolate(mode='area') calls; the window is summed, then multiplied by the weight)
 *        bilinear  num = max((2 o + 1) in - out, 0), den = 2 out, i0 = num div den, t = (num mod den) / den (one fp32 division):
 *                  weights 1 - t, t on i0, i0 + 1
 *        bicubic   num = (2 o + 1) in - out (may be negative), i0 = floor(num / den), t = (num - i0 den) / den, A = -0.75:
 *                  ((A (t + 1) - 5 A) (t + 1) + 8 A) (t + 1) - 4 A,  ((A + 2) t - (A + 3)) t t + 1,  the second at 1 - t,  the first
 *                  at 2 - t, on i0 - 1 .. i0 + 2; t and the four polynomials in double, each weight rounded to fp32 once
 *      Indices are clamped to 0 .. in - 1; two taps that clamp onto the same pixel add.  The forward adds the products of a pass in
 *      double and rounds once per pass (along x, then along y); the backward's sums are fp32 fused multiply-adds in index order.  This is F.interpolate(align_corners=False) of
 *      modes 'bilinear' and 'bicubic' (no antialias) and mode 'area'.  A non-finite input value reaches the outputs whose taps read it
 *      (a tap of weight 0 included, as in torch) and no others.
 *      SISR_E_BADARG before any HIP call for null pointers, sizes < 1, x and y (or the mode table and y) sharing a byte, a mode outside
 *      0 .. 2 given to the HOST table, weights of the draw that are negative, not finite or sum to 0, B < 1, rank outside [0, 65536);
 *      SISR_E_TOOBIG for N C, H W, h w or the workgroup count above INT32_MAX.  Tiles shrink with the ratio until a workgroup's staged
 *      block fits 64 KB of LDS.  SISR_E_UNSUPPORTED, from BOTH directions alike and before the launch, when not even a 1 x 1 tile fits:
 *      a down-scaling with about (H / h + 2) (W / w + 3) > 16000 or an up-scaling with about (4 h / H + 2) (4 w / W + 3) > 16000.
 *      Every ratio up to 16 per axis, up or down, is served. ------------------------------------------------------------------------ */
enum { SISR_RESIZE_AREA = 0, SISR_RESIZE_BILINEAR = 1, SISR_RESIZE_BICUBIC = 2 };
#define SISR_RESIZE_MAX_TAPS 64
/* HOST, no HIP call: the rows of R as the kernels compute them (one __host__ __device__ text).  Row o has count[o] weights
 * w[o][0 .. count[o] - 1] on the UNCLAMPED input indices first[o] .. first[o] + count[o] - 1 (bicubic: first may be -2, when
 * up-scaling, and the last index may reach in + 1; bilinear: the last may reach in); a reader clamps them to 0 .. in - 1 and adds
 * taps that meet.  first, count:
 * [out] int32; w: [out][SISR_RESIZE_MAX_TAPS], zeros behind the row's weights.  SISR_RESIZE_MAX_TAPS bounds this table only: an
 * area window longer than it is SISR_E_UNSUPPORTED here, while the kernels loop over a window of any length. */
int sisr_resize_taps_host(int32_t mode, int32_t in_size, int32_t out_size, int32_t *first, int32_t *count, float *w);
/* One launch: a workgroup per output tile (16 x 64, halved until it fits) and plane; the tile's taps, the input footprint and the
 * row-filtered footprint live in LDS. */
int sisr_resize_fwd(const float *x, const int32_t *modes_dev, float *y, int32_t N, int32_t C, int32_t H, int32_t W, int32_t h, int32_t w,
                    void *stream);
/* dx [N][C][H][W] = R_h^T dy R_w, the exact transpose (clamped border taps fold onto the border pixel), in gather form: every input
 * pixel sums the outputs that read it in index order.  One launch, no atomics, no zero-fill, every element of dx stored, the same
 * bits on every call. */
int sisr_resize_bwd(const float *dy, const int32_t *modes_dev, float *dx, int32_t N, int32_t C, int32_t H, int32_t W, int32_t h, int32_t w,
                    void *stream);
/* One workgroup: t = *drawn_step_dev is READ and not advanced (the pattern of sisr_jpeg_tables: the launch shares the step a stage's
 * draw stored).  Sample b: counter {t low, t high, b, 0xFE090000 | rank}, u0 = ((r0 >> 8) + 0.5) 2^-24 in fp32; with
 * p_i = weight_i / ((p_area + p_bilinear) + p_bicubic) in fp32, the mode is the first i with p_i > 0 and u0 <= p_0 + .. + p_i (fp32,
 * added in index order; u0 above the rounded sum: the last mode with p_i > 0).  modes_dev [B] int32. */
int sisr_resize_modes_draw(const int64_t *drawn_step_dev, uint64_t seed, int32_t rank, int32_t B, float p_area, float p_bilinear,
                           float p_bicubic, int32_t *modes_dev, void *stream);
/* HOST: the same text for step t >= 0 into host memory, no GPU involved. */
int sisr_resize_modes_host(int64_t t, uint64_t seed, int32_t rank, int32_t B, float p_area, float p_bilinear, float p_bicubic,
                           int32_t *modes_host);

/* ---- NIQE, the no-reference image quality score of Mittal, Soundararajan and Bovik (IEEE SPL 2013), as BasicSR's calculate_niqe
 *      defines it: the 36 features of every block of an image, and the score against a pristine model.
 *      img: fp32 [N][C][H][W], contiguous, C 1 or 3; block even, 16 .. SISR_NIQE_MAX_BLOCK; everything after the image is read is double.
 *      1. View and plane: strip `crop` pixels from every side; v = (x - lo) k with k = 255 / (hi - lo) (lo, hi taken as double);
 *         C == 3: Y = 16 + ((65.481 R + 128.553 G) + 24.966 B) / 255 (BT.601 studio range, MATLAB's rgb2ycbcr), C == 1: Y = v; the
 *         products and sums rounded as written (nothing fused); Y = rint(Y), half to even; the top-left
 *         floor(h / block) block x floor(w / block) block pixels are kept (nb = their blocks, row-major) and nothing else is seen.
 *      2. Two scales: scale 1 is that plane with blocks of `block`; scale 2 the plane down-scaled by 2 with blocks of block / 2:
 *         along each axis out[i] = sum_{k=0..7} w_k in[2 i - 3 + k], w = (-3, -9, 29, 111, 111, 29, -9, -3) / 256 (MATLAB's
 *         antialiased bicubic at exactly 1/2), an index outside the axis mirrored with the edge pixel repeated (-1 -> 0, L -> L - 1),
 *         no clamp of the result (the sums are exact in double, so the order of the axes does not matter).
 *      3. MSCN: g_k ~ exp(-k^2 / (2 (7/6)^2)), k = -3 .. 3, normalised to sum 1; the 2-D window is g_i g_j; the border is replicated.
 *         mu = g * I, sigma = sqrt(|g * I^2 - mu^2|), mscn = (I - mu) / (sigma + 1), computed from the moments ABOUT THE PIXEL:
 *         m1 = sum g_i g_j (I_ij - I), m2 = sum g_i g_j (I_ij - I)^2, sigma = sqrt(|m2 - m1^2|), mscn = -m1 / (sigma + 1): the
 *         differences are exact, the variance loses no digits, and a constant 7 x 7 neighbourhood gives exactly 0.
 *      4. AGGD fit of a field f over one block: L = sqrt(mean f^2 over f < 0), R = sqrt(mean f^2 over f > 0), gamma = L / R,
 *         r = (mean |f|)^2 / mean f^2, Rhat = r (gamma^3 + 1) (gamma + 1) / (gamma^2 + 1)^2; alpha = alpha_j = 0.2 + 0.001 j with
 *         j = argmin_j (rho_j - Rhat)^2 over j = 0 .. SISR_NIQE_TABLE - 1 (first minimum; a NaN or infinite Rhat: j = 0, and every other
 *         number of that fit is a NaN), rho_j = Gamma(2 / alpha_j)^2 / (Gamma(1 / alpha_j) Gamma(3 / alpha_j)), strictly increasing;
 *         beta_l = L sqrt(Gamma(1 / alpha) / Gamma(3 / alpha)), beta_r likewise, m = (beta_r - beta_l) Gamma(2 / alpha) / Gamma(1 / alpha).
 *         tables: DEVICE double [4][SISR_NIQE_TABLE], built by the caller on the host: Gamma(1 / alpha_j), Gamma(2 / alpha_j),
 *         Gamma(3 / alpha_j) and rho_j formed from them.
 *      5. Features of a block, 18 per scale, scale 1 first: (alpha, (beta_l + beta_r) / 2) of the block's MSCN, then for the shifts
 *         (0, 1), (1, 0), (1, 1), (1, -1) the fit (alpha, m, beta_l, beta_r) of mscn roll(mscn, shift), the roll circular INSIDE the
 *         block; block (by, bx) of scale 2 is the block / 2 square at the same block coordinates of the down-scaled plane.
 *         sharp: the block's mean of sigma at scale 1.
 *      6. Score against (mu_p [36], cov_p [36][36], DEVICE doubles): mu_d = the column means over the blocks ignoring NaNs, cov_d = the
 *         unbiased covariance of the rows without a NaN, S = (cov_p + cov_d) / 2, d = mu_p - mu_d, score = sqrt(d^T S^-1 d) by a Cholesky
 *         factorisation in double (square-root-free, S = L D L^T: the same pivots); fewer than two complete rows, or a pivot that is
 *         not > 0, gives a NaN score (the pseudo-inverse of a singular S is not formed).
 *      Launches: sisr_niqe_features FOUR (plane, down-scale, one block launch per scale), sisr_niqe_score ONE, whatever N and nb are.
 *      No atomics, fixed-order sums, nothing read back by the host: the same bits on every call.
 *      SISR_E_BADARG before any HIP call for null pointers (sharp may be NULL), a workspace, feature, model or table pointer that is not
 *      8-byte aligned, N < 1, nb < 1, an odd block or one outside 16 .. SISR_NIQE_MAX_BLOCK, a non-finite or empty value range, a negative
 *      crop; SISR_E_UNSUPPORTED for C not 1 or 3 or a view smaller than one block; SISR_E_TOOBIG past INT32_MAX elements or N > 65535. */
#define SISR_NIQE_MAX_BLOCK 96
#define SISR_NIQE_FEATURES 36
#define SISR_NIQE_TABLE 9801
/* HOST: bytes of the workspace (the two planes and the score's row flags: one workspace serves both calls; the score alone needs
 * 4 N nb bytes); < 0: a status code */
int64_t sisr_niqe_ws_bytes(int32_t N, int32_t H, int32_t W, int32_t crop, int32_t block);
/* feat: double [N][nb][36]; sharp: float [N][nb] or NULL */
int sisr_niqe_features(const float *img, int32_t N, int32_t C, int32_t H, int32_t W, int32_t crop, float lo, float hi, int32_t block,
                       const double *tables, void *ws, double *feat, float *sharp, void *stream);
/* feat: double [N][nb][36] as sisr_niqe_features left it; score: float [N] */
int sisr_niqe_score(const double *feat, int32_t N, int32_t nb, const double *mu_p, const double *cov_p, void *ws, float *score,
                    void *stream);

/* ---- misc---------------------------------------------------------------------------------- */
/* ---- optimizer: fused multi-tensor Adam --------------------------------------------------
 * One launch performs torch.optim.Adam's update (amsgrad=False, maximize=False; config.py:292-294, stepped at
 * train.py:75,108) for every parameter of a network.  Table in DEVICE memory; block_start = running sum of
 * sisr_adam_blocks(numel) over the preceding entries; total_blocks = that sum over all entries.  The caller passes
 * lr (after any LambdaLR factor, config.py:170-180) and the bias corrections 1 - beta^t of the step being taken.
 * Tensors need only 4-byte alignment: 16-byte accesses are used when numel % 4 == 0 and every pointer the launch touches
 * (p, m, v and g for the steps, g for the sum of squares) is 16-byte aligned. */
typedef struct SisrAdamDesc {
    float *p, *m, *v;          /* parameter, exp_avg, exp_avg_sq (updated in place)            */
    const float *g;            /* gradient                                                      */
    int64_t numel;
    int64_t block_start;
} SisrAdamDesc;
int64_t sisr_adam_blocks(int64_t numel);
int sisr_adam_step(const SisrAdamDesc *table_dev, int32_t n, int64_t total_blocks, double lr, double beta1, double beta2,
                   double eps, double weight_decay, double bias_corr1, double bias_corr2, void *stream);

/* ---- the same step with its per-step scalars in DEVICE memory (capturable: DESIGN.md section 10) --------------
 * Nothing below takes a step count, a learning rate or a bias correction from the host, so the three launches can be
 * captured into a HIP graph and still advance on every replay.  Same table and block mapping as above.  Sequence per step:
 *   [sisr_adam_grad_sumsq]  only with a guard: one double partial of sum g^2 per workgroup into `partials`
 *                           (sisr_adam_norm_ws_doubles doubles; squares and sums in double, fixed order, no atomics);
 *   sisr_adam_prepare       one thread per tensor, any n.  With n_partials > 0 it first adds the partials in a fixed order and
 *                           derives norm, coef = min(1, max_norm / (norm + 1e-6)) (max_norm < 0: coef = 1) and skip =
 *                           skip_nonfinite && the fp32 norm is not finite; with write_ctrl it stores ctrl[4] = { fp32 norm,
 *                           fp32 coef, int32 skip, int32 running count of skipped steps }.  Then, unless skip, per tensor i:
 *                           t = *steps_dev[i] (fp32 count, torch's capturable layout); consts[2i] = lr / (1 - beta1^(t+1)),
 *                           consts[2i+1] = 1 / sqrt(1 - beta2^(t+1)), both in double and rounded to fp32 once;
 *                           *steps_dev[i] = t + 1.  lr_dev: ONE device scalar, fp32 or (lr_is_f64) fp64.
 *                           Several tables that share one norm: run every sum of squares into consecutive ranges of one
 *                           workspace first, then one prepare per table over the WHOLE range, write_ctrl on the first only.
 *   sisr_adam_step_dev      the update; g is multiplied by ctrl's coef before weight decay is added (the gradient tensor
 *                           is only read); when ctrl's skip flag is set the kernel exits before any store.
 * steps_dev: n device pointers in DEVICE memory; consts: 2 n floats; ctrl: 4 words, written only by the prepare launch.
 * SISR_E_BADARG before any HIP call for null pointers, n <= 0, total_blocks outside [1, 2^31) and betas outside [0, 1). */
int64_t sisr_adam_norm_ws_doubles(int64_t total_blocks);
int sisr_adam_grad_sumsq(const SisrAdamDesc *table_dev, int32_t n, int64_t total_blocks, double *partials, void *stream);
int sisr_adam_prepare(float *const *steps_dev, int32_t n, const void *lr_dev, int32_t lr_is_f64, double beta1, double beta2,
                      const double *partials, int64_t n_partials, double max_norm, int32_t skip_nonfinite, int32_t write_ctrl,
                      float *ctrl, float *consts, void *stream);
int sisr_adam_step_dev(const SisrAdamDesc *table_dev, int32_t n, int64_t total_blocks, const float *consts, const float *ctrl,
                       double beta1, double beta2, double eps, double weight_decay, void *stream);

/* ---- exponential moving average of a network's weights: fused, multi-tensor, capturable -----------
 * The averaged ("shadow") copy of every parameter and fp32 buffer of a network is updated by one launch; the update count and
 * the decay schedule live in DEVICE memory, so the launches can sit inside a captured HIP graph behind the capturable Adam step
 * and still advance on every replay.  Table in DEVICE memory, block mapping of SisrAdamDesc (block_start = running sum of
 * sisr_adam_blocks(numel), total_blocks = that sum).  mode 0 averages, mode 1 copies (BatchNorm running statistics, spectral-norm
 * u / v).  Tensors need only 4-byte alignment: 16-byte accesses are used when numel % 4 == 0 and both pointers are 16-byte aligned.
 *   sisr_ema_prepare   ONE thread, the only code that touches the count: n = *count_dev;
 *                      d = warmup > 0 ? min(decay, (1 + n) / (warmup + n)) : decay in double; ctrl = { fp32 (float)(1 - d),
 *                      int32 active = 1 }; *count_dev = n + 1.  With skip_flag_dev (the capturable Adam's skip word) non-zero:
 *                      active = 0 and nothing else is stored.
 *   sisr_ema_update    mode 0: ema += omd * (src - ema) (an element with src == ema keeps its bits); mode 1: ema = src, bit-copied;
 *                      src is only read; no store at all when ctrl's active word is 0.
 *   sisr_ema_swap      exchanges the bits of ema[i] and src[i], whatever the mode.
 * Plain vector stores, no atomics, nothing read back by the host.  SISR_E_BADARG before any HIP call for null pointers (the skip
 * flag may be null), n <= 0, total_blocks outside [1, 2^31), decay outside [0, 1) and warmup < 0 (NaNs included). */
typedef struct SisrEmaDesc {
    float *ema;                /* the averaged copy (updated in place)                          */
    float *src;                /* the live tensor (only sisr_ema_swap writes it)                */
    int64_t numel;
    int64_t block_start;
    int32_t mode;              /* 0: average, 1: copy                                           */
    int32_t pad;
} SisrEmaDesc;
int sisr_ema_prepare(int32_t *count_dev, double decay, double warmup, const int32_t *skip_flag_dev, float *ctrl, void *stream);
int sisr_ema_update(const SisrEmaDesc *table_dev, int32_t n, int64_t total_blocks, const float *ctrl, void *stream);
int sisr_ema_swap(const SisrEmaDesc *table_dev, int32_t n, int64_t total_blocks, void *stream);

/* sizeof() of the descriptor structs in declaration order (Conv, Wgrad, Weight, WeightGrad,
 * BnBwd, ConvPlan, DeepPlan, WgradDeepPlan, ImageRec) so a binding can verify its mirror of this header; returns the count. */
int sisr_struct_sizes(int32_t *out, int32_t cap);
int sisr_device_info(int32_t *n_cu, int32_t *lds_per_cu, char *arch, int32_t arch_len);
int sisr_mfma_selftest(float *out_dev /* >= 32*32 floats */, void *stream);
int sisr_tr16_selftest(int16_t *out_dev /* >= 64*8 shorts */, void *stream);
/* fetch-and-clear the calling thread's pending HIP error (e.g. after an abandoned stream capture) so that it is
 * not attributed to the next launch; returns the code that was pending (0: none) */
int sisr_clear_last_error(void);
const char *sisr_version(void);

#ifdef __cplusplus
}
#endif
#endif /* SISR_HIP_H */
