"""Seeded cases, float64 references, exactness budgets and derived bounds of the fp32-tensor kernel family -- conv_fwd.hip,
conv_wgrad.hip, conv_toimage.hip (f32 mode), wgrad_toimage.hip (f32) and the persistent conv_trunk_f32.hip / wgrad_trunk_f32.hip in
their two precisions 'fp32' (fp32 matrix instruction) and 'bf16x3' (bf16 matrix instruction over hi / lo pairs) -- everything of
tests/test_gpu_f32_exact.py that needs no device; tests/test_f32_cases_cpu.py checks the cases' own conditions.  The operand
builders, references and bounds of tests/bf16_cases.py are reused; what differs is the staged value: this family contracts the FP32
result of the prologue (operand().v and its fp32 evaluations), never its bf16 rounding.

Three tiers.
  A, grid operands (the fine and coarse grids of bf16_cases): every product and partial sum is exact in fp32 in any order, and a
     bf16-representable value splits as hi = x, lo = 0 -- both precisions must EQUAL the float64 reference.
  S, two-piece operands ('bf16x3' only): every staged value has 9 significant bits inside one binade, so hi = bf16(v) (8 bits, ties
     to even), lo = v - hi is one bit, representable, and hi + lo == v.  The kernel's contraction hi hi + hi lo + lo hi (the lo lo
     term is dropped by design) is then exact as long as sum |terms| stays below 2^22 steps of the finest of the three product
     grids: values are sparse (density per case) to keep it there.  Reference: the same three float64 convolutions.  A kernel that
     reads a wrong lo (a neighbouring channel, tap or pixel) or drops one differs by whole grid steps.  Prologue constants are
     powers of two and shifts zero, so the staged value keeps its bits: the inputs are the staged values with the prologue inverted.
  B, ordinary random fp32 operands (not bf16-representable), element by element (K terms, S = sum |a||w| + |bias| + |residual|):
       fp32     gamma_{K+2} S + P            P = sum |w| r u mag: the r <= 5 fp32 roundings of the prologue, relative to the magnitude
                                             `mag` of its terms (operand().mag); every evaluation differs in the last bit, so there is
                                             no ambiguous share here
       bf16x3   gamma_{3K+2} S + P (1 + 2^-8) + D + R    against the full float64 conv of the fp32 staged values:
                                             D = sum |lo_x||lo_w|, the dropped term; R = sum |x||w - hi_w - lo_w| + |x - hi_x - lo_x||w|,
                                             what rounding lo loses -- both from the CPU emulation of the split; 2^-8 P: the split of
                                             the kernel's own fp32 value instead of v moves hi + lo by at most the perturbation itself
                                             and |lo| by as much, |lo_w| <= 2^-9 |w| (second order)
     bias gradient: (pixels + 5) u sum mag (any order); reduction rows: (D_chain + r) u sum |terms| as in bf16_cases.

Chain lengths, counted from the kernels:
  conv_fwd.hip        statistics: two passes over the tile.  A lane adds MSUB x 16 <= 32 values, + 1 lane-half shuffle + 3 wave adds
                      = a chain of 36, divided by the count; sum (y - mean)^2 the same chain.  No Chan merge: (36, 0).  One row per
                      pixel tile.  No BatchNorm-backward epilogue (the descriptor is refused).
  conv_trunk_f32.hip  statistics: a lane keeps sum (y - shift) and sum (y - shift)^2 in ONE chain each over the 16 T values of its T
                      tiles, shift = the mean of its first 16; lane halves, then the three other waves in sequence: 4 Chan merges
                      with f = 1/2, 1/2, 1/3, 1/4 -- the shifted form of stats_bounds counts 4 u per merge where f = 1/2 and 8 u
                      otherwise, so the four are passed as 8.  shift is the mean of 16 of the lane's 16 T values (not of 32 T as in
                      conv_trunk.hip): s2 <= (1 + T) M2 by the same Cauchy-Schwarz step, so stats_bounds, which forms 1 + 2 T' from
                      its tiles_per_row T', is given T' = T / 2.  One row per pixel-tile stream.
                      reductions: a lane's chain of 16 T terms + 1 shuffle + 2 levels (w0 + w1) + (w2 + w3) = 16 T + 3, + 4 roundings
                      of a term; the slope sum: 16 T + 1 shuffle + a chain over 128 partials = 16 T + 129, + 4.  Two rows per stream.
"""
import functools
from types import SimpleNamespace as NS

import torch
import torch.nn.functional as F

import bf16_cases as B
from bf16_cases import (ACT, ACT_BWD, AFFINE_ACT, BNACT_BWD, BNBWD, BUDGET, NONE, RES_AFFINE, TANH_BWD, U, bnb_terms, channel_stats,    # noqa: F401
                        choice, conv_dgrad, conv_fwd, conv_wgrad, gamma, grid, operand, rand, stats_bounds, step_of)

F32, F64 = torch.float32, torch.float64
PRECISIONS = ('fp32', 'bf16x3')
R_PRO = 5                                   # roundings of a prologue, contracted or not (as wgrad_case's bias bound)
# the max-norm tolerances these bounds stand beside (tests/test_gpu_kernels.py, tests/test_gpu_trunk_f32_walk.py)
MAXNORM_TOL = {('generic', 'conv'): 2e-4, ('generic', 'wgrad'): 2e-4, ('toimage', 'conv'): 2e-4, ('toimage', 'wgrad'): 2e-4,
               ('trunk', 'conv', 'fp32'): 1e-5, ('trunk', 'conv', 'bf16x3'): 4e-5, ('trunk', 'wgrad', 'fp32'): 1e-4,
               ('trunk', 'wgrad', 'bf16x3'): 1e-4}


def split(v):
    """the kernels' split of fp32 values (float64 tensor): hi = bf16(v), lo = bf16(v - hi), both round-to-nearest-even"""
    hi = B.bf(v.float()).double()
    return hi, B.bf((v - hi).float()).double()


def two_piece(shape, seed, exp, density, bits=9):
    """seeded values of `bits` significant bits in the binade [2^exp, 2^(exp + 1)), random signs; a share `density` is kept, the rest 0"""
    g = B._gen(seed)
    m = torch.randint(0, 2 ** (bits - 1), shape, generator=g).double()
    mag = (2 ** (bits - 1) + m) * 2.0 ** (exp - bits + 1)
    sign = torch.randint(0, 2, shape, generator=g).double() * 2 - 1
    keep = (torch.rand(shape, generator=g) < density).double()
    return (mag * sign * keep).to(F32)


def _unlrelu(v, slope):
    return v if slope is None else torch.where(v < 0, v / slope, v)


def split_operand(pro, shape, seed, density, no_slope=False):
    """inputs of operand() whose value AFTER prologue `pro` is a two_piece() tensor v (|v| in [1, 2)): the prologue inverted with
    power-of-two constants and zero shifts -> (kwargs, v)"""
    c = shape[1]
    v = two_piece(shape, seed, 0, density)
    k = {}
    sl = 0.5
    half_or_one = lambda s: choice((c,), [0.5, 1.0], s)
    bc = B._bc
    if pro == NONE:
        k['x1'] = v
    elif pro == ACT:
        k.update(x1=_unlrelu(v, sl), slope=sl)
    elif pro == AFFINE_ACT:
        pa = choice((c,), [0.5, 1.0, 2.0], seed + 1)
        k.update(x1=_unlrelu(v, sl) / bc(pa), pa=pa, pd=torch.zeros(c), slope=sl)
    elif pro == ACT_BWD:
        x2 = grid(shape, 0.25, 1.0, seed + 2)
        k.update(x1=torch.where(x2 > 0, v, v / sl), x2=x2, slope=sl)
    elif pro in (BNBWD, BNACT_BWD):
        pa = half_or_one(seed + 1)
        x2 = grid(shape, 0.25, 2.0, seed + 2)
        k.update(x2=x2, pa=pa, pb=torch.zeros(c), pd=torch.zeros(c))
        a = v / bc(pa)
        if pro == BNACT_BWD:
            ps, pt = half_or_one(seed + 3), grid((c,), 0.25, 1.0, seed + 4)
            a = torch.where(bc(ps) * x2 + bc(pt) > 0, a, a / sl)
            k.update(ps=ps, pt=pt, slope=sl)
        k['x1'] = a
    elif pro == RES_AFFINE:
        pa = half_or_one(seed + 1)
        first = torch.rand(shape, generator=B._gen(seed + 5)) < 0.5           # which of the two summands carries the element
        zero = torch.zeros_like(v)
        s = None if no_slope else sl
        k.update(x1=_unlrelu(torch.where(first, v, zero), s), x2=torch.where(first, zero, v) / bc(pa), pa=pa, pd=torch.zeros(c), slope=s)
    else:
        raise ValueError(pro)
    return k, v


def _geometry(role, geom, shuffle2):
    """-> (operand shape, contraction f(a, w, b) in the layout of the result, terms per element, shape of the result)"""
    n, cin, cout, k, stride, h, w = geom
    pad = k // 2
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    if role == 'fwd':
        post = B.pixel_shuffle2 if shuffle2 else (lambda t: t)
        f = lambda a, ww, bb: post(conv_fwd(a, ww, bb, stride, pad))
        return (n, cin, h, w), f, cin * k * k, (n, cout // 4, 2 * ho, 2 * wo) if shuffle2 else (n, cout, ho, wo)
    gshape = (n, cout // 4, 2 * ho, 2 * wo) if shuffle2 else (n, cout, ho, wo)
    view = (lambda a: F.pixel_unshuffle(a, 2)) if shuffle2 else (lambda a: a)
    return gshape, (lambda a, ww, bb: conv_dgrad(view(a), ww, stride, pad, (h, w))), cout * k * k, (n, cin, h, w)


@functools.lru_cache(maxsize=None)
def conv_case(role, geom, pro, tier, seed=0, res=False, bnb=None, coarse=False, bias=True, shuffle2=False, no_slope=False,
              density=(1.0 / 32, 1.0)):
    """One forward ('fwd') or data-gradient ('dgrad') launch on fp32 tensors; arguments as bf16_cases.conv_case.  tier 'grid' IS that
    function's case with un-rounded storage (on a grid the staged fp32 and bf16 values coincide).  tier 'split': density = (operand,
    weights).  -> namespace with k, op, a (the staged float64 values), w, b, res, ref, oshape, terms; grid / split: step, budget;
    split: lo_share = (operand, weights); rand: s, bound[precision], e_acc[precision]"""
    if tier == 'grid':
        c = B.conv_case(role, geom, pro, 'grid', seed=seed, res=res, bnb=bnb, coarse=coarse, rounded=False, out_bf16=False, bias=bias,
                        shuffle2=shuffle2, no_slope=no_slope)
        c = NS(**vars(c))
        c.a, c.shuffle2 = c.op.v, shuffle2
        return c
    n, cin, cout, k, stride, h, w = geom
    ashape, f, terms, oshape = _geometry(role, geom, shuffle2)
    out = NS(role=role, geom=geom, pro=pro, tier=tier, terms=terms, oshape=oshape, shuffle2=shuffle2)
    if tier == 'split':
        kw, v = split_operand(pro, ashape, 2000 + seed, density[0], no_slope)
        wt = two_piece((cout, cin, k, k), 1000 + seed, -4, density[1])
        b = grid((cout,), 2.0 ** -6, 0.5, 1001 + seed) if bias and role == 'fwd' else None
        r = grid(oshape, 2.0 ** -4, 0.5, 3000 + seed) if res else None
    else:
        kw, _ = B.make_operand(pro, ashape, 'rand', 2000 + seed, rounded=False, no_slope=no_slope)
        wt, b = B.make_weights(cout, cin, k, 'rand', 1000 + seed, bias=bias and role == 'fwd')
        r = rand(oshape, 3000 + seed) if res else None
    op = operand(pro, **kw)
    a, w64 = op.v, wt.double()
    b64, r64 = (None if b is None else b.double()), (0.0 if r is None else r.double())
    absb = None if b is None else b64.abs()
    (ah, al), (wh, wl) = split(a), split(w64)
    out.__dict__.update(k=kw, op=op, a=a, w=wt, b=b, res=r, hi_lo=((ah, al), (wh, wl)))
    if tier == 'split':
        out.target = v.double()
        out.ref = f(ah, wh, b64) + f(ah, wl, None) + f(al, wh, None) + r64
        s = f(ah.abs(), wh.abs(), absb) + f(ah.abs(), wl.abs(), None) + f(al.abs(), wh.abs(), None) + abs(r64)
        steps = [step_of(ah) * step_of(wh), step_of(ah) * step_of(wl), step_of(al) * step_of(wh)] + [step_of(t) for t in (b, r) if t is not None]
        out.step = min(steps)
        out.budget = float(s.max()) / out.step
        out.lo_share = tuple(float((lo != 0).double().sum() / max(float((t != 0).sum()), 1.0)) for lo, t in ((al, a), (wl, w64)))
        # every output element sees a cross term
        out.cross = f(ah.abs(), wl.abs(), None) + f(al.abs(), wh.abs(), None)
        full = f(a, w64, b64) + r64
        out.dropped = float((full - out.ref).abs().max())          # the lo lo term: what an "all four products" kernel would add
    else:
        out.ref = f(a, w64, b64) + r64
        out.s = s = f(a.abs(), w64.abs(), absb) + abs(r64)
        p = f(R_PRO * U * op.mag, w64.abs(), None)
        d = f(al.abs(), wl.abs(), None)
        rr = f(a.abs(), (w64 - wh - wl).abs(), None) + f((a - ah - al).abs(), w64.abs(), None)
        out.bound = {'fp32': gamma(terms + 2) * s + p, 'bf16x3': gamma(3 * terms + 2) * s + p * (1 + 2.0 ** -8) + d + rr}
        out.e_acc = out.bound
    if bnb is not None:
        assert role == 'dgrad'
        xb, k4, bslope = B.make_bnb(oshape, 'grid' if tier == 'split' else tier, 4000 + seed, bnb == 'act')
        if tier != 'split':
            xb = rand(oshape, 4000 + seed, 2.0)                  # (fp32 tensors: not bf16-representable)
        out.bnb = NS(x=xb, k4=k4, slope=bslope, terms=bnb_terms(out.ref, xb, k4, bslope))
    return out


def emulated(case, precision):
    """the case's contraction evaluated by torch in fp32 on the staged values: as it is ('fp32'), or the three products of the split
    ('bf16x3')"""
    _, f, _, _ = _geometry(case.role, case.geom, case.shuffle2)
    b = case.b
    a, w = case.a.float(), case.w
    if precision == 'fp32':
        y = f(a, w, b)
    else:
        (ah, al), (wh, wl) = split(case.a), split(case.w.double())
        y = f(al.float(), wh.float(), None) + f(ah.float(), wl.float(), None) + f(ah.float(), wh.float(), b)
    return y if case.res is None else y + case.res


def bnb_reference(case, precision, depth_c, depth_s):
    """bf16_cases.bnb_reference with the accumulator error of `precision` carried through the terms (tier B)"""
    c = NS(**vars(case))
    c.tier = 'grid' if case.tier in ('grid', 'split') else 'rand'
    if c.tier == 'rand':
        c.e_acc = case.e_acc[precision]
    return B.bnb_reference(c, depth_c, depth_s)


@functools.lru_cache(maxsize=None)
def wgrad_case(geom, xpro, gpro, tier, seed=0, shuffle2=False, density=(1.0 / 8, 1.0 / 8)):
    """One weight-gradient launch on fp32 tensors: dW = sum over pixels of x'(pixel + tap) (x) dy'(pixel), the bias gradient the sum of
    dy'.  tier 'grid': bf16_cases.wgrad_case with un-rounded storage.  'split': both operands two-piece, density = (x, dy)"""
    if tier == 'grid':
        c = NS(**vars(B.wgrad_case(geom, xpro, gpro, 'grid', seed=seed, coarse=True, x_rounded=False, g_rounded=False, shuffle2=shuffle2)))
        return c
    n, cin, cout, k, stride, h, w = geom
    pad = k // 2
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    gshape = (n, cout // 4, 2 * ho, 2 * wo) if shuffle2 else (n, cout, ho, wo)
    if tier == 'split':
        kx, vx = split_operand(xpro, (n, cin, h, w), 5000 + seed, density[0])
        kg, vg = split_operand(gpro, gshape, 6000 + seed, density[1])
    else:
        kx, _ = B.make_operand(xpro, (n, cin, h, w), 'rand', 5000 + seed, rounded=False)
        kg, _ = B.make_operand(gpro, gshape, 'rand', 6000 + seed, rounded=False)
    xo, go = operand(xpro, **kx), operand(gpro, **kg)
    if shuffle2:                                              # elementwise prologue first, then the view
        go = NS(**{name: F.pixel_unshuffle(getattr(go, name), 2) for name in ('v', 'q', 'alt', 'mag')}, ambiguous=go.ambiguous,
                evals=[F.pixel_unshuffle(e, 2) for e in go.evals])
        if tier == 'split':
            vg = F.pixel_unshuffle(vg, 2)
    wshape = (cout, cin, k, k)
    f = lambda a, g: conv_wgrad(a, g, wshape, stride, pad)
    x, g = xo.v, go.v
    (xh, xl), (gh, gl) = split(x), split(g)
    dims, pix = (0, 2, 3), n * ho * wo
    out = NS(geom=geom, xpro=xpro, gpro=gpro, tier=tier, kx=kx, kg=kg, xo=xo, go=go, terms=pix, gb_ref=g.sum(dims), hi_lo=((xh, xl), (gh, gl)))
    if tier == 'split':
        out.targets = (vx.double(), vg.double())
        out.ref = f(xh, gh) + f(xh, gl) + f(xl, gh)
        s = f(xh.abs(), gh.abs()) + f(xh.abs(), gl.abs()) + f(xl.abs(), gh.abs())
        out.step = min(step_of(xh) * step_of(gh), step_of(xh) * step_of(gl), step_of(xl) * step_of(gh))
        out.budget = max(float(s.max()) / out.step, float(g.abs().sum(dims).max()) / step_of(g))
        out.lo_share = tuple(float((lo != 0).double().sum() / max(float((t != 0).sum()), 1.0)) for lo, t in ((xl, x), (gl, g)))
        out.cross = f(xh.abs(), gl.abs()) + f(xl.abs(), gh.abs())
        out.dropped = float((f(x, g) - out.ref).abs().max())
    else:
        out.ref = f(x, g)
        out.s = s = f(x.abs(), g.abs())
        ex, eg = R_PRO * U * xo.mag, R_PRO * U * go.mag
        p = f(ex, g.abs()) + f(x.abs(), eg) + f(ex, eg)
        d = f(xl.abs(), gl.abs())
        rr = f(x.abs(), (g - gh - gl).abs()) + f((x - xh - xl).abs(), g.abs())
        out.bound = {'fp32': gamma(pix + 2) * s + p, 'bf16x3': gamma(3 * pix + 2) * s + p * (1 + 2.0 ** -8) + d + rr}
        out.gb_bound = (pix + R_PRO) * U * go.mag.sum(dims)
    return out


def emulated_wgrad(case, precision):
    n, cin, cout, k, stride, h, w = case.geom
    f = lambda a, g: conv_wgrad(a, g, (cout, cin, k, k), stride, k // 2)
    if precision == 'fp32':
        return f(case.xo.v.float(), case.go.v.float())
    (xh, xl), (gh, gl) = split(case.xo.v), split(case.go.v)
    return f(xl.float(), gh.float()) + f(xh.float(), gl.float()) + f(xh.float(), gh.float())


# ---- chain lengths (see the module text) -------------------------------------------------------------------------------------------
GENERIC_STAT_CHAIN = (36, 0, 0)


def trunk_stat_chain(tiles):
    return 16 * tiles, 8, tiles / 2.0


def trunk_bnb_depth(tiles):
    return 16 * tiles + 3 + 4, 16 * tiles + 129 + 4


# ---- the case tables of tests/test_gpu_f32_exact.py ---------------------------------------------------------------------------------
# trunk shapes (n, h, w[, cap]) of tests/test_gpu_trunk_f32_walk.py -> (pixel-tile streams, tiles of the longest walk): the fp32 kernel
# pairs workgroups, so cap / 2 slots: sisr_equal_shares(tiles, slots) = (ceil(tiles / rounds), rounds = ceil(tiles / slots))
TRUNK_WALK = {(1, 8, 16): (1, 1), (1, 16, 16, 2): (1, 2), (1, 24, 16, 2): (1, 3), (3, 24, 48, 10): (5, 6), (2, 16, 32): (8, 1)}
WALK_SHAPES = list(TRUNK_WALK)
WALK27 = WALK_SHAPES[3]
UP_SHAPES = [(1, 8, 16), (2, 16, 32, 4)]
# the channel-ragged geometries of test_gpu_kernels.CONV_CASES
RAGGED_CHANNELS = [(2, 3, 64, 9, 1, 12, 12), (2, 16, 16, 3, 1, 9, 8), (1, 4, 4, 3, 1, 16, 16), (1, 1, 3, 3, 1, 16, 16), (2, 48, 40, 3, 1, 7, 9)]
GENERIC = B.GENERIC + RAGGED_CHANNELS
IMAGE_IN = RAGGED_CHANNELS[0]                    # the first conv: its operand is the NCHW fp32 image
FWD_PROS = B.FWD_PROS
DG_CROSS = [(pro, res) for pro in (NONE, BNBWD, BNACT_BWD, ACT_BWD) for res in (False, True)]       # (pro, res) of DG_COMBOS + DG_REST
# (prologue, residual, reductions) of test_data_gradient_walk
TRUNK_DG = [(BNBWD, False, None), (BNBWD, True, 'plain'), (BNACT_BWD, True, 'act'), (BNACT_BWD, False, 'plain'), (BNACT_BWD, True, None),
            (BNBWD, False, 'act')]
# tier S densities (operand, weights) of the 64 -> 64 / 64 -> 256 convs and (x, dy) of their weight gradients, by pixel count:
# tests/test_f32_cases_cpu.py measures every case's budget
def conv_density(terms, sparse_w=False):
    """18 operand values per output element under dense weights (1 / 32 of the trunk conv's 576 terms, 1 / 128 of the 2304 of the upscale
    conv's data gradient), or 72 under weights of density 1 / 4"""
    return (72.0 / terms, 0.25) if sparse_w else (18.0 / terms, 1.0)


def wg_density(shape):
    pix = shape[0] * shape[1] * shape[2]
    return (1.0 / 4, 1.0 / 4) if pix <= 512 else (1.0 / 8, 1.0 / 8) if pix <= 1024 else (1.0 / 16, 1.0 / 16)


class Run(NS):
    def __repr__(self):
        names = B.PRO_NAMES
        if self.role == 'wgrad':
            pro = names[self.xpro] + '+' + names[self.gpro]
        else:
            pro = names[self.pro]
        return '-'.join(str(v).replace(' ', '') for v in (self.family, self.role, self.shape, pro, self.tier, self.precision,
                                                          'res' if self.res else '', self.bnb or '', 'shuffle' if self.shuffle2 else '',
                                                          self.tag) if v != '')


def _mk(family, role, shape, pro, tier, precision, res=False, bnb=None, shuffle2=False, tag='', **kw):
    return Run(family=family, role=role, shape=shape, pro=pro, tier=tier, precision=precision, res=res, bnb=bnb, shuffle2=shuffle2,
               tag=tag, **kw)


def _seeded(runs, stride):
    """one seed per case: the two precisions of a grid or random case share operands and reference"""
    seeds = {}
    for x in runs:
        key = repr(NS(**{**vars(x), 'precision': ''}))
        x.seed = seeds.setdefault(key, stride * len(seeds))
    return runs


def _tiers(family):
    """(tier, precision) pairs: the split is the trunk kernels'; the generic kernels have one precision"""
    if family == 'trunk':
        return [('grid', 'fp32'), ('grid', 'bf16x3'), ('split', 'bf16x3')]
    return [('grid', 'fp32')]


def _conv_runs():
    r = []
    for tier, pr in _tiers('trunk'):
        for sh in WALK_SHAPES:
            r += [_mk('trunk', 'fwd', sh, pro, tier, pr) for pro in FWD_PROS]
            r += [_mk('trunk', 'fwd', sh, RES_AFFINE, tier, pr, tag=t) for t in ('slope', 'noslope')]
            r += [_mk('trunk', 'dgrad', sh, pro, tier, pr, res, bnb) for pro, res, bnb in TRUNK_DG]
        for sh in UP_SHAPES:
            r += [_mk('trunk', 'fwd', sh, pro, tier, pr, shuffle2=True) for pro in (NONE, AFFINE_ACT)]
            r += [_mk('trunk', 'dgrad', sh, ACT_BWD, tier, pr, res, shuffle2=True) for res in (False, True)]
    # tier S, the other density: sparse weights under a denser operand
    r += [_mk('trunk', 'fwd', WALK27, NONE, 'split', 'bf16x3', tag='sparse_w'), _mk('trunk', 'dgrad', WALK27, BNBWD, 'split', 'bf16x3', tag='sparse_w')]
    for pr in PRECISIONS:
        r += [_mk('trunk', 'fwd', WALK27, pro, 'rand', pr) for pro in (AFFINE_ACT, RES_AFFINE)]
        r += [_mk('trunk', 'dgrad', WALK27, BNACT_BWD, 'rand', pr, True, 'act')]
        r += [_mk('trunk', 'fwd', UP_SHAPES[1], AFFINE_ACT, 'rand', pr, shuffle2=True), _mk('trunk', 'dgrad', UP_SHAPES[1], ACT_BWD, 'rand', pr, True, shuffle2=True)]
    for g in GENERIC:
        nchw_in = g == IMAGE_IN
        r += [_mk('generic', 'fwd', g, pro, 'grid', 'fp32', tag='image_in' if nchw_in else '') for pro in ([NONE] if nchw_in else FWD_PROS)]
        r += [_mk('generic', 'dgrad', g, pro, 'grid', 'fp32', res) for pro, res in DG_CROSS]
    r.append(_mk('generic', 'fwd', B.UPSCALE, ACT, 'grid', 'fp32', shuffle2=True))
    r += [_mk('generic', 'dgrad', B.UPSCALE, ACT_BWD, 'grid', 'fp32', res, shuffle2=True) for res in (False, True)]
    r += [_mk('generic', 'fwd', B.LAST_CONV, ACT, 'grid', 'fp32', tag=t) for t in ('nchw', 'tanh')]
    r += [_mk('generic', 'fwd', B.RAGGED, AFFINE_ACT, 'rand', 'fp32'), _mk('generic', 'dgrad', B.RAGGED, BNACT_BWD, 'rand', 'fp32', True),
          _mk('generic', 'dgrad', B.GENERIC[4], BNBWD, 'rand', 'fp32', True, tag='stride2')]
    for sh in B.TOIMAGE:
        r += [_mk('toimage', 'fwd', sh, pro, 'grid', 'fp32', tag=t) for pro in (NONE, ACT) for t in ('', 'tanh')]
    r += [_mk('toimage', 'fwd', B.TOIMAGE[1], ACT, 'rand', 'fp32', tag=t) for t in ('', 'tanh')]
    return _seeded(r, 13)


def run_geom(r):
    sh = r.shape
    if r.family == 'generic':
        return sh
    n, h, w = sh[:3]
    if r.family == 'trunk':
        return (n, 64, 256 if r.shuffle2 or r.tag == 'up' else 64, 3, 1, h, w)
    return (n, 64, 3, 3, 1, h, w)                          # toimage


def image_out_run(r):
    return r.family == 'toimage' or r.tag in ('nchw', 'tanh')


def run_case(r):
    geom = run_geom(r)
    terms = 9 * (geom[1] if r.role == 'fwd' else geom[2])
    return conv_case(r.role, geom, r.pro, r.tier, seed=r.seed, res=r.res, bnb=r.bnb, shuffle2=r.shuffle2, no_slope=r.tag == 'noslope',
                     density=conv_density(terms, r.tag == 'sparse_w'))


CONV_RUNS = _conv_runs()


def stat_run(r):
    """the forward launch also writes BatchNorm statistics rows (the PixelShuffle and NCHW stores have no such epilogue)"""
    return r.role == 'fwd' and r.family in ('generic', 'trunk') and not r.shuffle2 and not image_out_run(r)


def run_stat_chain(r):
    return trunk_stat_chain(TRUNK_WALK[r.shape][1]) if r.family == 'trunk' else GENERIC_STAT_CHAIN


def _wg(family, shape, xpro, gpro, tier, precision, tag=''):
    return Run(family=family, role='wgrad', shape=shape, xpro=xpro, gpro=gpro, tier=tier, precision=precision, res=False, bnb=None,
               shuffle2=tag == 'up', tag=tag)


def _wg_runs():
    r = []
    for tier, pr in _tiers('trunk'):
        for sh in WALK_SHAPES:
            r += [_wg('trunk', sh, xp, gp, tier, pr) for xp, gp in B.WG_TRUNK_PAIRS]
        r += [_wg('trunk', sh, ACT, ACT_BWD, tier, pr, 'up') for sh in UP_SHAPES]
    for pr in PRECISIONS:
        r += [_wg('trunk', WALK27, AFFINE_ACT, BNACT_BWD, 'rand', pr), _wg('trunk', UP_SHAPES[1], ACT, ACT_BWD, 'rand', pr, 'up')]
    for g in GENERIC:
        r += [_wg('generic', g, xp, gp, 'grid', 'fp32', 'image_in' if g == IMAGE_IN else '') for xp, gp in (B.WG_PAIRS[:1] if g == IMAGE_IN else B.WG_PAIRS)]
    r.append(_wg('generic', B.PADDED, NONE, TANH_BWD, 'grid', 'fp32', 'padded'))
    r.append(_wg('generic', B.RAGGED, AFFINE_ACT, BNACT_BWD, 'rand', 'fp32'))
    r += [_wg('toimage', B.WG_THIN[0], xp, gp, 'grid', 'fp32') for xp, gp in ((NONE, NONE), (ACT, TANH_BWD), (NONE, TANH_BWD), (ACT, NONE))]
    r.append(_wg('toimage', B.WG_THIN[0], ACT, TANH_BWD, 'rand', 'fp32'))
    return _seeded(r, 17)


def wg_case(r):
    return wgrad_case(run_geom(r), r.xpro, r.gpro, r.tier, seed=r.seed, shuffle2=r.tag == 'up', density=wg_density(r.shape))


WG_RUNS = _wg_runs()
# three layers in one sisr_wgrad_trunk_f32_batch launch
TRUNK_BATCH = {(tier, pr): [Run(family='trunk', role='wgrad', shape=(2, 16, 32), xpro=AFFINE_ACT, gpro=BNBWD, tier=tier, precision=pr, res=False,
                                bnb=None, shuffle2=False, tag='batch', seed=9000 + i) for i in range(3)] for tier, pr in _tiers('trunk')}


def all_wg_runs():
    return WG_RUNS + [r for rs in TRUNK_BATCH.values() for r in rs]
