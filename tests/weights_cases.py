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
