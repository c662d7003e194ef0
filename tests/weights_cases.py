"""Seeded inputs, float64 references and derived bounds of the weight-side kernels (csrc/spectral.hip): everything of
tests/test_gpu_weights.py that needs no device, so that tests/test_weights_args_cpu.py can check the inputs' conditions (the
quotient-rule cap, the NaN padding, the closed form of the tile count) where there is no GPU.

u = 2^-24 is the fp32 unit round-off.  hipcc contracts `a += b * c` into one fused multiply-add, so a chain of D such steps rounds D
times; every bound below is first order in u (the second-order terms are below 1e-5 of the bound at the chain lengths used here).
BS = 9: block_sum's additions on the longest chain -- 6 of the wave butterfly, 3 over the four wave totals (0 + the first is exact)."""
import ctypes as C
import functools
import math

import torch

from gpu_helpers import pkg

U = 2.0 ** -24
BS = 9
SN_RB, SN_CB, BLOCK = 16, 1024, 256                    # csrc/spectral.hip, csrc/sisr_dev.h
F32 = torch.float32


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _uniform(shape, seed, scale=1.0):
    return ((torch.rand(shape, generator=_gen(seed)) * 2 - 1) * scale).to(F32)


def cdiv(a, b):
    return (a + b - 1) // b


# ---- a. power iteration ---------------------------------------------------------------------------------------------------------
# (Cout, Cin, K): the branch each one reaches is named in tests/test_gpu_weights.py
SN_SHAPES = [(64, 32, 3), (40, 24, 3), (64, 3, 3), (16, 3, 9), (3, 64, 3), (32, 96, 3), (48, 128, 3), (272, 32, 1), (20, 1, 3)]


@functools.lru_cache(maxsize=None)
def sn_inputs(shape, seed=0):
    """(W as a [rows, cols] matrix, u, v): fp32, u and v unit vectors as torch.nn.utils.spectral_norm keeps them"""
    cout, cin, k = shape
    rows, cols = cout, cin * k * k
    base = 1000 + 16 * SN_SHAPES.index(shape) + 3 * seed if shape in SN_SHAPES else 5000 + seed
    w = _uniform((rows, cols), base, 0.1)
    u = torch.nn.functional.normalize(torch.randn(rows, generator=_gen(base + 1)), dim=0).to(F32)
    v = torch.nn.functional.normalize(torch.randn(cols, generator=_gen(base + 2)), dim=0).to(F32)
    return w, u, v


def sn_work_floats(rows, cols):
    return cdiv(rows, SN_RB) * cols + rows


def _normalised_bound(x64, e_x, d_sumsq):
    """|fl(x_got * fl(1 / fl(sqrt(fl(sum x_got^2))))) - x64 / |x64||, first order, for |x_got - x64| <= e_x element-wise:
         e_x / n                        the element's own error, n = |x64|
       + |x64| / n * |e_x|_2 / n        the norm moves by at most |x_got - x64|_2 <= |e_x|_2
       + |x64| / n * (d_sumsq / 2 + 3) u  the sum of squares (all terms positive: d_sumsq roundings, relative, halved by the root),
                                          one sqrt, one reciprocal, one product -- each correctly rounded"""
    n = x64.norm()
    return e_x / n + x64.abs() / n * (e_x.norm() / n + (d_sumsq / 2 + 3) * U)


def sn_reference(w, u_in, v_got, u_got, training):
    """float64 references and bounds of one power-iteration step, stage by stage (every stage starts from what the kernel returned
    for the stage before, so no bound carries an earlier stage's error):
       t     = W^T u_in                 D_t = min(16, rows) FMAs of a row block + ceil(rows / 16) additions over the row blocks
       v     = t / |t|                  _normalised_bound with the t bound, sum of squares: ceil(cols / 256) FMAs + BS
       s     = W v_got                  the kernel forms fl(fl(W t_got) * iv) while v_got = fl(t_got * iv): the dot's D_s =
                                        ceil(cols / 64) FMAs + 6 butterfly additions, + 2 for those two products
                                        (evaluation mode: s = W v, iv = 1 exactly: D_s alone)
       u     = s / |s|                  _normalised_bound with the s bound, sum of squares: ceil(rows / 256) FMAs + BS
       sigma = u_got . s                sum |u_got| e_s + (ceil(rows / 256) + BS) u sum |u_got s|
    -> dict of (reference, bound)"""
    rows, cols = w.shape
    w64, out = w.double(), {}
    if training:
        u64 = u_in.double()
        t64 = w64.t() @ u64
        e_t = (min(SN_RB, rows) + cdiv(rows, SN_RB)) * U * (w64.abs().t() @ u64.abs())
        out['t'] = (t64, e_t)
        out['v'] = (t64 / t64.norm(), _normalised_bound(t64, e_t, cdiv(cols, BLOCK) + BS))
    vg = v_got.double()
    s64 = w64 @ vg
    e_s = (cdiv(cols, 64) + 6 + (2 if training else 0)) * U * (w64.abs() @ vg.abs())
    if training:
        out['u'] = (s64 / s64.norm(), _normalised_bound(s64, e_s, cdiv(rows, BLOCK) + BS))
    ug = u_got.double()
    e_sig = (ug.abs() * e_s).sum() + (cdiv(rows, BLOCK) + BS) * U * (ug * s64).abs().sum()
    out['sigma'] = ((ug @ s64).reshape(1), e_sig.reshape(1))
    return out


def sn_rows_dot(w, vec_got):
    """what sn_w_v_kernel leaves in the scratch: W vec_got (vec = the t the kernel formed, or v in evaluation mode), a wave per row:
    lane chains of ceil(cols / 64) FMAs + 6 butterfly additions -> (reference, bound)"""
    w64, x = w.double(), vec_got.double()
    return w64 @ x, (cdiv(w.shape[1], 64) + 6) * U * (w64.abs() @ x.abs())


def sn_sigma_from_rows(u_got, s_got):
    """evaluation mode: sigma = u . s with the s the kernel left in the scratch (iv = 1): ceil(rows / 256) FMAs + BS"""
    ug, sg = u_got.double(), s_got.double()
    return (ug @ sg).reshape(1), ((cdiv(ug.numel(), BLOCK) + BS) * U * (ug * sg).abs().sum()).reshape(1)


# ---- b. gradient epilogue -------------------------------------------------------------------------------------------------------
# (Cout, Cin, K, shuffle2)
GEN_L0 = [(64, 64, 3, 0), (40, 24, 3, 1), (48, 40, 3, 0), (64, 3, 9, 0), (3, 64, 3, 0), (16, 1, 3, 0), (64, 64, 1, 0)]
GEN_L1 = [(256, 64, 3, 1), (4, 64, 3, 0)]
FAST = [(64, 64, 3, 0), (96, 32, 3, 0), (32, 96, 3, 0)]
FAST_TABLE = [(128, 64, 3, 0), (32, 32, 3, 0), (64, 128, 3, 0)]
SIGMA = 0.37
PLAN_FIELDS = ('CK', 'PS', 'KROWP', 'n_chunk', 'CoutPad')


def wgrad_plan(cout, cin, k, layout):
    """the slab geometry of the weight-gradient kernels (host-only planners of the library; 2 x 16 x 16 maps, stride 1)"""
    L = pkg('_lib')
    g = L.WgradDesc()
    g.N, g.H, g.W, g.Cin, g.Ho, g.Wo, g.Cout = 2, 16, 16, cin, 16, 16, cout
    g.KH = g.KW = k
    g.stride, g.pad_y, g.pad_x = 1, k // 2, k // 2
    fn = L.lib().sisr_wgrad_plan_bf16 if layout == 1 else L.lib().sisr_wgrad_plan
    assert fn(C.byref(g), 512) == 0
    return {n: getattr(g, n) for n in PLAN_FIELDS}


def tiles_closed_form(cout, cin, k, ck):
    """sisr_weights_grad_tiles as include/sisr_hip.h states it: ck = 32 for layout 1, the plan's CK otherwise -> (tiles, taps per tile)"""
    taps = k * k
    tg = max(1, min(taps, 32 // min(ck, cin)))
    return cdiv(cout, 32) * cdiv(cin, ck) * cdiv(taps, tg), tg


def packed_order(cout, shuffle2):
    """perm[cp] = the original output channel of packed channel cp (SisrWeightDesc.shuffle2: (i, j)-major for PixelShuffle(2))"""
    cp = torch.arange(cout)
    if not shuffle2:
        return cp
    cq = cout // 4
    return (cp % cq) * 4 + cp // cq


class GradCase:
    """one weight of an epilogue table: G, W_orig, u, v, sigma, the packed slab (NaN in every padding slot) and bias, the float64
    reference (G - (<G, W_orig> / sigma) u v^T) / sigma and what its bound needs"""

    def __init__(self, shape, layout, seed, plan_cout=None):
        cout, cin, k, shuffle2 = shape
        self.shape, self.layout = shape, layout
        self.cout, self.cin, self.k, self.shuffle2 = cout, cin, k, shuffle2
        taps = k * k
        self.cols = cols = cin * taps
        self.plan = wgrad_plan(plan_cout or cout, cin, k, layout)     # (plan_cout: a slab planned for more output channels)
        ck = 32 if layout == 1 else self.plan['CK']
        self.n_tiles, self.tg = tiles_closed_form(cout, cin, k, ck)
        self.nci = min(ck, cin)
        w = _uniform((cout, cin, k, k), seed, 0.1)
        r = _uniform((cout, cin, k, k), seed + 1)
        r = r * (w.double().norm() / r.double().norm()).float()          # |R|_F = |W_orig|_F
        self.w, self.g = w, (w + r).to(F32)
        # u, v: arbitrary, no unit vectors -- magnitudes in [0.5, 1.5] with random signs (no entry near zero: the rank-one term
        # is then a visible share of EVERY element), scaled so that rho lands near 0.5
        sg = lambda n, s: torch.where(torch.rand(n, generator=_gen(s)) < 0.5, -1.0, 1.0)
        u = (torch.rand(cout, generator=_gen(seed + 2)) + 0.5) * sg(cout, seed + 3)
        v = (torch.rand(cols, generator=_gen(seed + 4)) + 0.5) * sg(cols, seed + 5)
        g64, w64 = self.g.double(), w.double()
        self.sigma = float(torch.tensor(SIGMA, dtype=F32))
        self.dot = float((g64 * w64).sum())
        self.dot_abs = float((g64 * w64).abs().sum())
        rho0 = abs(self.dot / self.sigma) * float(u.double().norm() * v.double().norm()) / float(g64.norm())
        c = math.sqrt(0.5 / rho0)
        self.u, self.v = (u * c).to(F32), (v * c).to(F32)
        uv = torch.outer(self.u.double(), self.v.double()).reshape(cout, cin, k, k)
        self.uv = uv
        self.t = self.dot / self.sigma * uv
        self.rho = float(self.t.norm() / g64.norm())
        self.ref = (g64 - self.t) / self.sigma
        # packed gradient and bias
        P = self.plan
        perm = packed_order(cout, shuffle2)
        gp = self.g[perm]                                               # [cp][ci][r][s]
        if layout == 1:
            assert cin % 32 == 0 and P['n_chunk'] == cin // 32
            slab = torch.full((P['n_chunk'], taps, 32, P['CoutPad']), float('nan'))
            slab[:, :, :, :cout] = gp.reshape(cout, P['n_chunk'], 32, taps).permute(1, 3, 2, 0)
        else:
            assert P['n_chunk'] == cdiv(cin, P['CK']) and k * P['PS'] <= P['KROWP'] and P['CK'] <= P['PS']
            slab = torch.full((P['n_chunk'], k, P['KROWP'], P['CoutPad']), float('nan'))
            for ch in range(P['n_chunk']):
                ci0 = ch * P['CK']
                n = min(P['CK'], cin - ci0)
                dst = slab[ch, :, :k * P['PS']].view(k, k, P['PS'], P['CoutPad'])     # [r][s][cl][cp]
                dst[:, :, :n, :cout] = gp[:, ci0:ci0 + n].permute(2, 3, 1, 0)
        self.slab = slab.reshape(-1)
        self.n_pad = int(torch.isnan(self.slab).sum())
        b = _uniform((cout,), seed + 6)
        self.bias = b                                                   # the reference of grad_bias, original channel order
        self.bias_pk = torch.full((P['CoutPad'],), float('nan'))
        self.bias_pk[:cout] = b[perm]

    def check_inputs(self):
        """the conditions on the seeded inputs: a wrong quotient-rule term cannot hide (rho >= 0.25) and every padding slot of the
        slab -- the columns >= Cout, the krow slots between and behind the channels -- holds a NaN"""
        assert self.rho >= 0.25, (self.shape, self.rho)
        assert self.n_pad == self.slab.numel() - self.cout * self.cols, (self.shape, self.n_pad)
        assert int(torch.isnan(self.bias_pk).sum()) == self.plan['CoutPad'] - self.cout
        assert self.sigma > 0 and abs(float(self.u.double().norm()) - 1) > 0.05 and abs(float(self.v.double().norm()) - 1) > 0.05

    def dot_chain(self, fast):
        """additions on the longest chain of <G, W_orig>, counted from the kernels, -> (one tile's partial, the whole dot)
        generic: a thread's ceil(rows * 32 / 256) FMAs over its tile (rows = taps per tile x channels of the chunk) + BS;
                 then ceil(tiles / 256) additions per thread over the tile partials + BS
        fast:    per float4 item a product, an FMA, the pair sum and the accumulation: 3 in front of a chain of 9 items, + BS;
                 then ceil(tiles / 256) + BS over the 32 x 32-channel tiles"""
        if fast:
            tiles = cdiv(self.cout, 32) * (self.cin // 32)
            tile = 3 + 9 + BS
        else:
            tiles = self.n_tiles
            tile = cdiv(self.tg * self.nci * 32, BLOCK) + BS
        return tile, tile + cdiv(tiles, BLOCK) + BS

    def tile_dots(self, fast):
        """float64 <G, W_orig> and sum |terms| per tile, in dot_work order
        generic: tile = (tap group, channel chunk, 32 PACKED couts), index (tgi * chunks + chunk) * cout tiles + cot
        fast:    tile = (32 couts, 32 channels, all taps), index cb * (Cin / 32) + kb"""
        taps = self.k * self.k
        prod = (self.g.double() * self.w.double()).reshape(self.cout, self.cin, taps)
        co, ci, tap = torch.meshgrid(torch.arange(self.cout), torch.arange(self.cin), torch.arange(taps), indexing='ij')
        if fast:
            tile, n = (co // 32) * (self.cin // 32) + ci // 32, cdiv(self.cout, 32) * (self.cin // 32)
        else:
            ck = 32 if self.layout == 1 else self.plan['CK']
            cp_of = torch.empty(self.cout, dtype=torch.long)
            cp_of[packed_order(self.cout, self.shuffle2)] = torch.arange(self.cout)
            n_cot, n_chunk = cdiv(self.cout, 32), cdiv(self.cin, ck)
            tile, n = ((tap // self.tg) * n_chunk + ci // ck) * n_cot + cp_of[co] // 32, self.n_tiles
        dots = torch.zeros(n, dtype=torch.float64).index_add_(0, tile.reshape(-1), prod.reshape(-1))
        sums = torch.zeros(n, dtype=torch.float64).index_add_(0, tile.reshape(-1), prod.abs().reshape(-1))
        return dots, sums

    def grad_bound(self, fast):
        """2^-23 (|g| + |gw u v|) / sigma for the subtraction and the scaling by 1 / sigma, + the dot's error x |u v| / sigma^2.
        The dot reaches the subtraction through three more roundings (generic: / sigma, * u, * v; fast: sigma * sigma, the
        division, * u): they are counted on its chain."""
        e_dot = (self.dot_chain(fast)[1] + 3) * U * self.dot_abs
        return 2 * U * (self.g.double().abs() + self.t.abs()) / self.sigma + e_dot * self.uv.abs() / self.sigma ** 2


@functools.lru_cache(maxsize=None)
def grad_case(shape, layout, seed):
    return GradCase(shape, layout, seed)


def all_grad_cases():
    """every (shape, layout, seed) the GPU tests build -- test_weights_args_cpu.py checks their conditions without a device"""
    out = []
    for i, s in enumerate(GEN_L0):
        out.append((s, 0, 100 + 10 * i))
    for i, s in enumerate(GEN_L1 + FAST + FAST_TABLE):
        out.append((s, 1, 300 + 10 * i))
    return out


def case_of(shape, layout):
    for s, lay, seed in all_grad_cases():
        if s == shape and lay == layout:
            return grad_case(s, lay, seed)
    raise KeyError((shape, layout))


# ---- c. packed weight images ----------------------------------------------------------------------------------------------------
# Every image the pack kernels write is ONE gather under one tap map, laid out in one of five storage orders (include/sisr_hip.h):
# element (out, in, r', s') of an image holds forward tap (R0y + Sy r', R0x + Sx s') of the weight -- zero outside it -- with
#   (R0, S) = (0, +1)        the forward image                      out = packed cout, in = cin
#             (K - 1, -1)    the stride-1 data gradient             out = cin, in = packed cout  ("transposed")
#             (c_R0, -2)     one parity class of a stride-2 one     out = cin, in = cout
# (build, [(cin, cout, k, stride, shuffle2, h, w)]), n = 2: what each layer reaches is asserted by tests/test_gpu_weight_images.py
IMAGE_CASES = {
    'fp32': [(64, 64, 3, 1, 0, 16, 16), (64, 256, 3, 1, 1, 16, 16), (3, 64, 9, 1, 0, 16, 16), (64, 3, 3, 1, 0, 16, 16),
             (40, 48, 3, 1, 0, 16, 16), (64, 64, 3, 2, 0, 16, 16)],
    'bf16x3': [(64, 64, 3, 1, 0, 16, 16)],
    'bf16': [(64, 64, 3, 1, 0, 16, 16), (64, 256, 3, 1, 1, 16, 16), (64, 3, 3, 1, 0, 16, 16), (32, 64, 3, 2, 0, 16, 16),
             (64, 64, 3, 2, 0, 16, 16), (64, 64, 3, 2, 0, 15, 15), (64, 64, 3, 1, 0, 12, 12)],
}
IMG_F32, IMG_BF16, IMG_DEEP = 0, 1, 2
WLDS_WORDS = 2 * 2 * 9 * 32 * 36
I32, BF16 = torch.int32, torch.bfloat16


class ImageSpec:
    """one image of a layer as the host planner decided it.  fmt: IMG_*; transposed: out = cin; taps = (KH', KW', R0y, Sy, R0x, Sx);
    plan: the SisrConvPlan fields of the role's descriptor (fp32 and bf16 orders); copy: LDS-order mode (fp32) or lane-order copy
    (bf16); row_taps: taps per row of the conv_deep.hip row format; old_slots: fp32 slots by the formulas of the engine before
    the library answered the question itself"""

    def __init__(self, name, fmt, transposed, taps, plan=None, copy=0, row_taps=0, old_slots=0):
        self.name, self.fmt, self.transposed, self.taps, self.plan = name, fmt, transposed, taps, plan
        self.copy, self.row_taps, self.old_slots = int(copy), row_taps, old_slots


def image_specs(E, p):
    """[ImageSpec | None] x 5 of one Prepared (plans, kinds, lanes, ldsimg; no device): forward, then the stride-1 data gradient or
    the four parity classes of a stride-2 one"""
    gm, (f, d, _) = p.ref.geom, p.plans
    k = gm.k

    def spec(name, desc, kind, taps, transposed, lanes=False, ldsimg=0, row_taps=None):
        plan = {n: getattr(desc.plan, n) for n in PLAN_FIELDS}
        if E.Kind(kind).deep:
            rows = row_taps or desc.KW
            old = (desc.deep.wimg_elems + 1) // 2 if row_taps is None else ((gm.cout // 32) * taps[0] * gm.cin * 72 + 1) // 2
            return ImageSpec(name, IMG_DEEP, transposed, taps, row_taps=rows, old_slots=old)
        if kind == E.Kind.BF16:
            return ImageSpec(name, IMG_BF16, transposed, taps, plan, lanes, old_slots=((desc.plan.wpk_elems + 1) // 2) * (2 if lanes else 1))
        return ImageSpec(name, IMG_F32, transposed, taps, plan, ldsimg, old_slots=desc.plan.wpk_elems + (WLDS_WORDS if ldsimg else 0))
    out = [spec('fwd', f, p.kinds[0], (k, k, 0, 1, 0, 1), False, p.lanes[0], p.ldsimg[0])] + [None] * 4
    shape = E._dgrad_shape(d)
    if shape == E.DG_CONV:
        out[1] = spec('dgrad', d, p.kinds[1], (k, k, k - 1, -1, k - 1, -1), True, p.lanes[1], p.ldsimg[1])
    elif shape == E.DG_X4:
        for c, t in enumerate(d.classes):
            out[1 + c] = spec('dgrad class %d' % c, d.desc, E.Kind.DEEP, (t.kh, t.kw, t.r0y, -2, t.r0x, -2), True, row_taps=2)
    elif shape == E.DG_CLASSES:
        for c, cl in enumerate(d):
            if cl is not None:
                out[1 + c] = spec('dgrad class %d' % c, cl.desc, cl.kind, (cl.desc.KH, cl.desc.KW, cl.r0y, -2, cl.r0x, -2), True)
    return out


def image_values(w4, shuffle2, transposed, taps):
    """the one gather: V[out][in][r'][s'] = w4[cout][cin][R0y + Sy r'][R0x + Sx s'] or 0 outside the weight, cout in packed order"""
    cout, cin, kh_w, kw_w = w4.shape
    kh, kw, r0y, sy, r0x, sx = taps
    wp = w4[packed_order(cout, shuffle2)]
    v = torch.zeros(cout, cin, kh, kw, dtype=F32)
    for rp in range(kh):
        for sp in range(kw):
            r, s = r0y + sy * rp, r0x + sx * sp
            if 0 <= r < kh_w and 0 <= s < kw_w:
                v[:, :, rp, sp] = wp[:, :, r, s]
    return v.transpose(0, 1).contiguous() if transposed else v


def order_f32(v, plan):
    """fp32 [chunk of CK in][r'][out, CoutPad][krow = s' * PS + (in - chunk * CK), KROWP]; every other slot zero"""
    n_out, n_in, kh, kw = v.shape
    CK, PS, KROWP, n_chunk, CoutPad = (plan[n] for n in PLAN_FIELDS)
    assert n_chunk == cdiv(n_in, CK) and kw * PS <= KROWP and CK <= PS and n_out <= CoutPad
    out = torch.zeros(n_chunk, kh, CoutPad, KROWP, dtype=F32)
    for ch in range(n_chunk):
        n = min(CK, n_in - ch * CK)
        dst = out[ch, :, :, :kw * PS].view(kh, CoutPad, kw, PS)
        dst[:, :n_out, :, :n] = v[:, ch * CK:ch * CK + n].permute(2, 0, 3, 1)
    return out.reshape(-1)


def order_bf16(v, plan):
    """bf16 [chunk of CK in][out, CoutPad][tap * CK + (in - chunk * CK)], RNE; rows out >= the channel count zero"""
    n_out, n_in, kh, kw = v.shape
    CK, CoutPad = plan['CK'], plan['CoutPad']
    assert n_in % CK == 0 and n_out <= CoutPad and plan['n_chunk'] == n_in // CK and plan['KROWP'] == kh * kw * CK
    out = torch.zeros(n_in // CK, CoutPad, kh * kw, CK, dtype=F32)
    out[:, :n_out] = v.reshape(n_out, n_in // CK, CK, kh * kw).permute(1, 0, 3, 2)
    return out.reshape(-1).to(BF16)


def order_lanes(v, plan):
    """the persistent trunk kernels' load order: [32-out block][tap][k slice j][lane = kk * 32 + out][8] bf16, in-channel
    (j >> 1) * 32 + (j & 1) * 16 + 8 kk + el"""
    n_out, n_in, kh, kw = v.shape
    CoutPad = plan['CoutPad']
    assert (n_in, kh, kw) == (64, 3, 3) and CoutPad % 32 == 0
    vp = torch.zeros(CoutPad, 64, 9, dtype=F32)
    vp[:n_out] = v.reshape(n_out, 64, 9)
    blk, tap, j, lane, el = torch.meshgrid(torch.arange(CoutPad // 32), torch.arange(9), torch.arange(4), torch.arange(64),
                                           torch.arange(8), indexing='ij')
    return vp[blk * 32 + (lane & 31), (j >> 1) * 32 + (j & 1) * 16 + 8 * (lane >> 5) + el, tap].reshape(-1).to(BF16)


def _bits16(t):
    return t.to(BF16).view(torch.int16).to(torch.int64) & 0xffff


def _word(lo16, hi16):
    """two 16-bit patterns (int64) -> the int32 with the same 32 bits"""
    x = lo16 | (hi16 << 16)
    return (x - ((x >> 31) << 32)).to(I32)


def order_lds(v, mode):
    """the fp32-tensor trunk conv's LDS order: 32-bit words [out half][in half q][tap][out 32][32 + 4]; mode 1: word wd < 32 the fp32
    value of in-channel 32 q + wd; mode 2: words 0..15 the RNE bf16 heads of in-channels (32 q + 2 m, + 1) (low, high half),
    words 16..31 the bf16 of what the heads leave; words 32..35 zero"""
    assert tuple(v.shape) == (64, 64, 3, 3) and mode in (1, 2)
    x = v.reshape(2, 32, 2, 32, 9).permute(0, 2, 4, 1, 3).contiguous()              # [hc][q][tap][co][in 32]
    out = torch.zeros(2, 2, 9, 32, 36, dtype=I32)
    if mode == 1:
        out[..., :32] = x.view(I32)
    else:
        hi = x.to(BF16)
        lo = (x - hi.float()).to(BF16)
        for half, t in ((0, hi), (16, lo)):
            b = _bits16(t)
            out[..., half:half + 16] = _word(b[..., 0::2], b[..., 1::2])
    return out.reshape(-1)


def order_deep(v, row_taps):
    """conv_deep.hip rows: bf16 [chunk of 32 in][r'][out][row_taps * 32 + 8], element s' * 32 + (in - chunk * 32); the taps a row
    has no s' for and the 8 padding elements zero"""
    n_out, n_in, kh, kw = v.shape
    assert n_in % 32 == 0 and kw <= row_taps
    out = torch.zeros(n_in // 32, kh, n_out, row_taps * 32 + 8, dtype=F32)
    out[..., :kw * 32] = v.reshape(n_out, n_in // 32, 32, kh, kw).permute(1, 3, 0, 4, 2).reshape(n_in // 32, kh, n_out, kw * 32)
    return out.reshape(-1).to(BF16)


def _slots(t):
    """any storage order as the 32-bit slots of the fp32 buffer it lives in"""
    if t.dtype == BF16:
        assert t.numel() % 2 == 0
    return t.contiguous().view(I32)


def expected_image(spec, w4, inv, shuffle2):
    """the 32-bit slots of one image: w4 the OIHW weight, inv = fl(1 / sigma) as an fp32 tensor (None: W_orig itself).
    fl32(W_orig * inv): one IEEE product per element -> (slots, elements of the standard order that hold a weight)"""
    scaled = w4 if inv is None else w4 * inv
    v = image_values(scaled, shuffle2, spec.transposed, spec.taps)
    if spec.fmt == IMG_DEEP:
        std = order_deep(v, spec.row_taps)
        parts = [std]
    elif spec.fmt == IMG_BF16:
        std = order_bf16(v, spec.plan)
        parts = [std] + ([order_lanes(v, spec.plan)] if spec.copy else [])
    else:
        std = order_f32(v, spec.plan)
        parts = [std] + ([order_lds(v, spec.copy)] if spec.copy else [])
    return torch.cat([_slots(x) for x in parts]), std


def image_layers(E, build):
    """the layers of IMAGE_CASES[build] planned under that build: [(geometry, (n, h, w), Prepared of _layout_weights)]"""
    before = E.PRECISION
    E.set_precision(build)
    try:
        out = []
        for cin, cout, k, stride, shuffle2, h, w in IMAGE_CASES[build]:
            gm = E.ConvGeom(cin, cout, k, stride, shuffle2=bool(shuffle2))
            ref = E.ConvRef(gm, None, None)
            out.append((gm, (2, h, w), E._layout_weights([(ref, 2, h, w)], True)[0][0]))
        return out
    finally:
        E.set_precision(before)


def check_reach(E, build, i, p):
    """what layer i of IMAGE_CASES[build] must reach for its images to cover the format they are listed for (host planner facts)"""
    K = E.Kind
    f, d, _ = p.plans
    shape = E._dgrad_shape(d)
    plan = {n: getattr(f.plan, n) for n in PLAN_FIELDS}
    what = (build, i, tuple(int(k) for k in p.kinds), p.lanes, p.ldsimg, shape, plan)
    if build in ('fp32', 'bf16x3'):
        assert p.kinds[0] == K.F32 and p.kinds[1] == K.F32 and p.lanes == (False, False), what
    if build == 'bf16x3':
        assert shape == E.DG_CONV and p.ldsimg == (2, 2), what
    elif build == 'fp32':
        if i == 0:
            assert shape == E.DG_CONV and p.ldsimg == (1, 1), what
        elif i in (1, 2, 3, 4):
            assert shape == E.DG_CONV and p.ldsimg == (0, 0), what
            if i == 2:
                assert (plan['CK'], plan['PS'], plan['KROWP']) == (3, 3, 28) and d.Cout == 3, what
            if i == 3:
                assert plan['CoutPad'] == 32, what
            if i == 4:
                assert (plan['CK'], plan['n_chunk']) == (32, 2), what
        else:
            assert shape == E.DG_CLASSES and all(c is not None and c.kind == K.F32 for c in d), what
            assert sorted((c.desc.KH, c.desc.KW) for c in d) == [(1, 1), (1, 2), (2, 1), (2, 2)], what
    else:
        if i == 0:
            assert p.kinds[:2] == (K.BF16, K.BF16) and shape == E.DG_CONV and p.lanes == (True, True), what
        elif i == 1:
            assert p.kinds[:2] == (K.BF16, K.BF16) and shape == E.DG_CONV and p.lanes == (True, False) and plan['CoutPad'] == 256, what
        elif i == 2:
            assert p.kinds[:2] == (K.BF16, K.F32) and shape == E.DG_CONV and plan['CoutPad'] > 3, what
        elif i == 3:
            assert p.kinds[0] == K.DEEP and shape == E.DG_CLASSES and all(c is not None and c.kind == K.BF16 for c in d), what
        elif i == 4:
            assert p.kinds[1] == K.DEEP_S2X4 and shape == E.DG_X4, what
        elif i == 5:
            assert shape == E.DG_CLASSES and all(c is not None and c.kind == K.DEEP for c in d), what
            assert sorted(c.desc.KW for c in d) == [1, 1, 2, 2], what
        else:
            assert p.kinds[:2] == (K.DEEP, K.DEEP) and shape == E.DG_CONV, what
        assert p.ldsimg == (0, 0), what
