// sisr_trunk_host.h -- host code shared by the four persistent trunk files: conv_trunk.hip / conv_trunk_f32.hip (the conv roles)
// and wgrad_trunk.hip / wgrad_trunk_f32.hip (the weight-gradient role).  The bf16-tensor and the fp32-tensor kernel of a role take
// the same layers and the same fusions; what differs is named by SisrTrunkKind, and each file keeps the conditions only its kernel
// has.  Host code only: include it after the kernels and their Args struct.
#pragma once
#include <cstring>
#include "sisr_host.h"

struct SisrTrunkKind {
    int th, tw;         // pixel tile
    bool bf16;          // tensor type of the operand and the output / gradient
    int px_bytes;       // bytes of a 64-channel pixel (tensors are addressed with 31-bit byte offsets; the upscale conv's 256 channels: 4x)
};

// ---- eligibility, conv roles.  0: not this geometry / these fusions, 1: forward role, 2: data-gradient role (the caller adds its
// kernel's conditions on res / bnb_x, on the plan, and the switches of its own; SISR_TRUNK is read by the caller) ----------------
static int sisr_trunk_conv_role(const SisrConvDesc* d, const SisrTrunkKind& k) {
    if (d->Cin != 64 || d->KH != 3 || d->KW != 3 || d->stride != 1 || d->pad_y != 1 || d->pad_x != 1) return 0;
    // Cout = 64 (trunk), or 256 stored through PixelShuffle(2) -- the upscale conv, forward role without statistics
    const bool up_off = sisr_switch_off("SISR_TRUNK_UP");      // A/B switch for the upscale conv alone
    const bool up = !up_off && d->Cout == 256 && d->y_mode == SISR_Y_NHWC_SHUFFLE2 && d->plan.CoutPad == 256 && !d->stat_part && !d->res &&
                    !d->bnb_part && !d->fin_stat &&
                    (d->pro_mode == SISR_PRO_NONE || d->pro_mode == SISR_PRO_ACT || d->pro_mode == SISR_PRO_AFFINE_ACT);
    if (!up && (d->Cout != 64 || d->y_mode != SISR_Y_NHWC)) return 0;
    if (d->x_mode != SISR_X_NHWC || (d->x_bf16 != 0) != k.bf16 || (d->y_bf16 != 0) != k.bf16) return 0;
    if (d->Ho != d->H || d->Wo != d->W || (d->H % k.th) || (d->W % k.tw)) return 0;
    if (!up && (d->y_sy != 1 || d->y_sx != 1 || d->y_oy || d->y_ox || d->y_H != d->Ho || d->y_W != d->Wo)) return 0;
    if (d->epi_act != SISR_EPI_NONE) return 0;
    if ((int64_t)d->N * d->H * d->W * k.px_bytes * (up ? 4 : 1) >= (1ll << 31)) return 0;
    if (d->N * (d->H / k.th) * (d->W / k.tw) >= 65536) return 0;
    const bool fwd_pro = d->pro_mode == SISR_PRO_NONE || d->pro_mode == SISR_PRO_ACT || d->pro_mode == SISR_PRO_AFFINE_ACT ||
                         (d->pro_mode == SISR_PRO_RES_AFFINE && d->x2 && d->x_out && ((d->pa && d->pd) || d->fin_stat));
    if (d->fin_stat && !((d->pro_mode == SISR_PRO_AFFINE_ACT || d->pro_mode == SISR_PRO_RES_AFFINE) && d->fin_cnt && d->fin_gamma &&
                         d->fin_beta && d->fin_rm && d->fin_rv && d->fin_k && d->fin_rows > 0))
        return 0;
    if (fwd_pro && !d->res && !d->bnb_part) return 1;           // forward role
    const bool bwd_pro = d->pro_mode == SISR_PRO_BNBWD || d->pro_mode == SISR_PRO_BNACT_BWD;
    return bwd_pro && !d->stat_part && !d->bias ? 2 : 0;        // data-gradient role
}

// ---- eligibility, weight-gradient role (the caller adds its kernel's plan check; SISR_TRUNK is read by the caller) --------------
static bool sisr_trunk_wgrad_ok(const SisrWgradDesc* d, const SisrTrunkKind& k) {
    if (sisr_switch_off("SISR_TRUNK_WGRAD")) return false;
    if (d->Cin != 64 || d->KH != 3 || d->KW != 3 || d->stride != 1 || d->pad_y != 1 || d->pad_x != 1) return false;
    // Cout = 64 (trunk: BatchNorm-backward gradient prologues), or 256 with the gradient stored shuffled and an
    // activation-backward prologue -- the upscale conv
    const bool up_off = sisr_switch_off("SISR_TRUNK_UP");      // A/B switch for the upscale conv alone
    const bool up = !up_off && d->Cout == 256 && d->g_mode == SISR_X_NHWC_UNSHUFFLE2 && d->CoutPad == 256 && d->gpro_mode == SISR_PRO_ACT_BWD;
    if (!up && (d->Cout != 64 || d->g_mode != SISR_X_NHWC || d->CoutPad != 64)) return false;
    if (d->x_mode != SISR_X_NHWC || (d->x_bf16 != 0) != k.bf16 || (d->g_bf16 != 0) != k.bf16) return false;
    if (d->Ho != d->H || d->Wo != d->W || (d->H % k.th) || (d->W % k.tw)) return false;
    if ((int64_t)d->N * d->H * d->W * k.px_bytes * (up ? 4 : 1) >= (1ll << 31)) return false;
    if (d->N * (d->H / k.th) * (d->W / k.tw) >= 65536) return false;
    const bool xp = d->pro_mode == SISR_PRO_NONE || d->pro_mode == SISR_PRO_ACT || d->pro_mode == SISR_PRO_AFFINE_ACT;
    const bool gp = up || d->gpro_mode == SISR_PRO_BNBWD || d->gpro_mode == SISR_PRO_BNACT_BWD;
    return xp && gp;
}

// workgroups of a weight-gradient launch: G cout groups (4 for the upscale conv) serve each tile stream; one slab per stream
static int sisr_trunk_wgrad_grid(const SisrWgradDesc* d, const SisrTrunkKind& k) {
    const int G = d->Cout == 256 ? 4 : 1;
    return G * sisr_equal_shares(d->N * (d->H / k.th) * (d->W / k.tw), sisr_cu_slots() / G);
}

// ---- Args filling: the fields the two Args structs of a role share ---------------------------------------------------------------
template <typename A>
static void sisr_trunk_conv_args(A& a, const SisrConvDesc* d, const SisrTrunkKind& k) {
    a.fin.stat = d->fin_stat; a.fin.cnt = d->fin_cnt; a.fin.gamma = d->fin_gamma; a.fin.beta = d->fin_beta;
    a.fin.rm = d->fin_rm; a.fin.rv = d->fin_rv; a.fin.k = d->fin_k; a.fin.rows = d->fin_rows; a.fin.momentum = d->fin_momentum; a.fin.eps = d->fin_eps;
    a.x1 = d->x1; a.x2 = d->x2; a.x_out = d->x_out; a.pa = d->pa; a.pb = d->pb; a.pd = d->pd; a.ps = d->ps; a.pt = d->pt;
    a.slope_p = d->pro_slope_p; a.slope = d->pro_slope;
    a.wpk = d->wpk; a.bias = d->bias; a.res = d->res; a.y = d->y; a.stat_part = d->stat_part; a.cnt_part = d->cnt_part;
    a.N = d->N; a.H = d->H; a.W = d->W;
    a.tiles_x = d->W / k.tw; a.per_img = (d->H / k.th) * a.tiles_x; a.total = d->N * a.per_img;
    a.m_tiles_x = fdiv_magic(a.tiles_x); a.m_per_img = fdiv_magic(a.per_img);
    a.cout_pad = d->Cout == 256 ? 256 : 64; a.shuffle = d->y_mode == SISR_Y_NHWC_SHUFFLE2 ? 1 : 0;
    a.bnb_x = d->bnb_x; a.bnb_scale = d->bnb_scale; a.bnb_shift = d->bnb_shift; a.bnb_mean = d->bnb_mean; a.bnb_invstd = d->bnb_invstd;
    a.bnb_slope_p = d->bnb_slope_p; a.bnb_slope = d->bnb_slope; a.bnb_act = d->bnb_act; a.bnb_part = d->bnb_part;
}

template <typename A>
static A sisr_trunk_wgrad_args(const SisrWgradDesc* d, const SisrTrunkKind& k) {
    A a{};
    a.x1 = d->x1; a.g1 = d->g1; a.g2 = d->g2;
    a.pa = d->pa; a.pd = d->pd; a.xslope_p = d->pro_slope_p; a.xslope = d->pro_slope;
    a.qa = d->qa; a.qb = d->qb; a.qd = d->qd; a.qs = d->qs; a.qt = d->qt;
    a.gslope_p = d->gpro_slope_p; a.gslope = d->gpro_slope;
    a.slab = d->slab; a.bias_slab = d->bias_slab; a.slab_stride = d->slab_stride;
    a.N = d->N; a.H = d->H; a.W = d->W;
    a.tiles_x = d->W / k.tw; a.per_img = (d->H / k.th) * a.tiles_x; a.total = d->N * a.per_img;
    a.m_tiles_x = fdiv_magic(a.tiles_x); a.m_per_img = fdiv_magic(a.per_img);
    a.xpro = d->pro_mode;
    a.glog = d->Cout == 256 ? 2 : 0; a.cout_pad = d->Cout == 256 ? 256 : 64; a.gshuffle = d->g_mode == SISR_X_NHWC_UNSHUFFLE2 ? 1 : 0;
    return a;
}

// operands the prologues of a weight-gradient launch read
static bool sisr_trunk_wgrad_operands(const SisrWgradDesc* d) {
    if (operand_needs_x2(d->gpro_mode) && !d->g2) return false;
    if (d->pro_mode == SISR_PRO_AFFINE_ACT && (!d->pa || !d->pd)) return false;
    return d->gpro_mode == SISR_PRO_ACT_BWD || (d->qa && d->qb && d->qd && (d->gpro_mode != SISR_PRO_BNACT_BWD || (d->qs && d->qt)));
}

// ---- a batch of trunk layers in one launch (the table kernels): Cout = 64, one gradient-prologue kind ----------------------------
// (same_split: the members must also agree on mfma_split, which picks the fp32 family's kernel)
static int sisr_trunk_wgrad_batch_check(const SisrWgradDesc* descs, int n, int (*eligible)(const SisrWgradDesc*), bool same_split) {
    if (!descs || n <= 0 || n > 4096) return SISR_E_BADARG;
    for (int i = 0; i < n; ++i) {
        const SisrWgradDesc* d = descs + i;
        if (!eligible(d) || d->Cout != 64 || d->gpro_mode != descs[0].gpro_mode) return SISR_E_BADARG;
        if (same_split && (d->mfma_split != 0) != (descs[0].mfma_split != 0)) return SISR_E_BADARG;
        if (!d->x1 || !d->g1 || !d->slab || d->slab_stride < d->slab_elems || !sisr_trunk_wgrad_operands(d)) return SISR_E_BADARG;
    }
    return 0;
}

// fills args_host (n * sizeof(A) bytes) with the kernel's view of the n descriptors; the caller copies it to device memory and
// passes that copy to the batch launch (the same staging route as every descriptor table of this library)
template <typename A>
static int sisr_trunk_wgrad_batch_args(const SisrWgradDesc* descs, int n, void* args_host, int (*check)(const SisrWgradDesc*, int),
                                       A (*fill)(const SisrWgradDesc*)) {
    if (!args_host) return SISR_E_BADARG;
    if (int e = check(descs, n)) return e;
    for (int i = 0; i < n; ++i) {
        const A a = fill(descs + i);
        std::memcpy(static_cast<unsigned char*>(args_host) + (size_t)i * sizeof(A), &a, sizeof(A));
    }
    return 0;
}
