"""Seeded inputs, lazy operands, float64 references, the exactness budget and the derived bounds of the bf16 matrix-core kernel
family -- everything of tests/test_gpu_bf16_exact.py that needs no device, so that tests/test_bf16_cases_cpu.py can check the
conditions that keep the GPU file from hiding a failure (budget, representability, ambiguous share, reference inside its own bound)
where there is no GPU.  Plain torch on the CPU; tensors are NCHW fp32 here, the GPU file changes layout and storage type.

Two tiers.
  A, grid operands: the matrix cores multiply bf16 values exactly and accumulate in fp32.  With every operand AFTER its prologue on
     a coarse binary grid, every partial sum of every summation order is an integer multiple of the product of the grid steps and
     stays below 2^24 of them: the fp32 result is exact, equal to the float64 reference bit for bit, whatever the tile / wave /
     K-split schedule.  budget() measures this per case; a case is exact only below 2^22 steps (two bits spare for an adder that
     aligns every addend of a 16-term block to the largest one).
  B, ordinary random operands: what separates the kernel from the float64 reference is the fp32 accumulation order
     (gamma_K * S, below) and the few staged values whose fp32 prologue result lies on the other side of a bf16 rounding tie when the
     compiler contracts a * x + d into one fused multiply-add (A, below).

u = 2^-24 is the fp32 unit round-off.  Bounds (element by element; `K` terms, S = sum |a||w| + |bias| + |residual|):
  contraction     gamma_K S + A,  gamma_K = K u / (1 - K u),  A = sum over the element's ambiguous operand values |w| |alt - chosen|
  bf16 output     + half a bf16 ulp of (|ref| + bound)
  a plain sum     whose longest chain of additions is D long (lane chain + tree levels), of terms that carry r roundings of their own:
                  (D + r) u sum |terms|  (first order; the classical bound of any summation tree of depth D)
  statistics      see stats_bounds(): the per-lane two-pass / shifted sums and the Chan merges of the three forward epilogues
"""
import functools
import math
from types import SimpleNamespace as NS

import torch
import torch.nn.functional as F

U = 2.0 ** -24
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
NONE, ACT, AFFINE_ACT, BNBWD, BNACT_BWD, ACT_BWD, TANH_BWD, RES_AFFINE = range(8)         # SISR_PRO_* of include/sisr_hip.h
TWO_TENSOR = (BNBWD, BNACT_BWD, ACT_BWD, TANH_BWD, RES_AFFINE)
BUDGET = 2.0 ** 22


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def grid(shape, step, limit, seed):
    """seeded integers in [-limit / step, limit / step] times step (step a power of two: every value is exact in bf16 when
    limit / step <= 256)"""
    k = int(round(limit / step))
    return (torch.randint(-k, k + 1, shape, generator=_gen(seed)).double() * step).to(F32)


def choice(shape, values, seed):
    v = torch.tensor(values, dtype=F32)
    return v[torch.randint(0, len(values), shape, generator=_gen(seed))]


def rand(shape, seed, scale=1.0):
    return ((torch.rand(shape, generator=_gen(seed)) * 2 - 1) * scale).to(F32)


def bf(t):
    return t.to(BF16).to(t.dtype)


def _bc(v):
    return v[None, :, None, None]


def _lrelu(v, s):
    return torch.where(v > 0, v, s * v)


# ---- lazy operands -----------------------------------------------------------------------------------------------------------------
def operand(pro, x1, x2=None, pa=None, pb=None, pd=None, ps=None, pt=None, slope=None):
    """The value a kernel's staging feeds to the contraction for operand (x1, x2) under prologue `pro` (SISR_PRO_*): computed in
    fp32, then rounded to bf16 with round-to-nearest-even.  All arguments fp32 (NCHW tensors, [C] constants, a python float slope).
      v     the un-rounded fp32 value (float64 tensor): the bias gradient is summed from it (stage_commit, SUM)
      q     the staged bf16 value (float64 tensor)
      alt   the bf16 value farthest from q that the staging may hold instead; != q only on AMBIGUOUS elements
      alts  every candidate
      mag   sum of the magnitudes of the prologue's terms (what an fp32 rounding of v is relative to)
      evals the two fp32 evaluations (2), (3) below before any bf16 rounding (what the fp32-tensor kernels stage: tests/f32_cases.py)
    How the compiler contracts a * b + c is its choice, so three evaluations are formed: (1) ONE rounding of the float64 value (the
    fully contracted limit) -> v; (2) every a * b + c one fused multiply-add, every other operation rounded (hipcc's default) -> q;
    (3) rounded after every operation (torch fp32).  An element where they stage different bf16 values -- the sign test of
    BNACT_BWD is part of each evaluation -- is ambiguous."""
    s32 = None if slope is None else torch.tensor(float(slope), dtype=F32)

    def f(cast, fma, s):
        a, b = cast(x1), cast(x2)
        ka, kb, kd, ks, kt = (None if t is None else _bc(cast(t)) for t in (pa, pb, pd, ps, pt))
        if pro == NONE:
            return a
        if pro == ACT:
            return _lrelu(a, s)
        if pro == AFFINE_ACT:
            return _lrelu(fma(ka, a, kd), s)
        if pro == BNBWD:
            return fma(kb, b, ka * a) + kd
        if pro == BNACT_BWD:
            return fma(kb, b, ka * torch.where(fma(ks, b, kt) > 0, a, s * a)) + kd
        if pro == ACT_BWD:
            return torch.where(b > 0, a, s * a)
        if pro == TANH_BWD:
            return a * fma(-b, b, torch.ones_like(b))
        if pro == RES_AFFINE:
            return (a if s is None else _lrelu(a, s)) + fma(ka, b, kd)
        raise ValueError(pro)

    d = lambda t: None if t is None else t.double()
    same = lambda t: t
    plain = lambda x, y, z: x * y + z
    fused = lambda x, y, z: (x.double() * y.double() + z.double()).float()       # (the product of two fp32 values is exact in float64)
    v = f(d, plain, None if s32 is None else float(s32)).float().double()
    e_fma, e_step = f(same, fused, s32).double(), f(same, plain, s32).double()
    q = bf(e_fma)
    alts = [bf(v), bf(e_step)]
    alt = torch.where((alts[0] - q).abs() >= (alts[1] - q).abs(), alts[0], alts[1])
    da, db = d(x1).abs(), None if x2 is None else d(x2).abs()
    k = lambda t: _bc(d(t)).abs()
    mag = {NONE: lambda: da, ACT: lambda: da, ACT_BWD: lambda: da, AFFINE_ACT: lambda: k(pa) * da + k(pd),
           BNBWD: lambda: k(pa) * da + k(pb) * db + k(pd), BNACT_BWD: lambda: k(pa) * da + k(pb) * db + k(pd),
           TANH_BWD: lambda: da * (1 + db ** 2), RES_AFFINE: lambda: da + k(pa) * db + k(pd)}[pro]()
    return NS(v=v, q=q, alt=alt, alts=[q] + alts, mag=mag, ambiguous=(q != alt), evals=[e_fma, e_step])


# ---- float64 references ------------------------------------------------------------------------------------------------------------
def pixel_shuffle2(t):
    """[N, 4C, H, W] -> [N, C, 2H, 2W]: out[n, c, 2h + i, 2w + j] = in[n, 4c + 2i + j, h, w]"""
    return F.pixel_shuffle(t, 2)


def conv_fwd(a, w, b, stride, pad):
    return F.conv2d(a, w, b, stride=stride, padding=pad)


def conv_dgrad(g, w, stride, pad, hw):
    """data gradient of conv2d(x [.., hw], w, stride, pad) for output gradient g"""
    ho, wo = g.shape[2:]
    k = w.shape[2]
    op = (hw[0] + 2 * pad - k - (ho - 1) * stride, hw[1] + 2 * pad - k - (wo - 1) * stride)
    return F.conv_transpose2d(g, w, stride=stride, padding=pad, output_padding=op)


def conv_wgrad(a, g, wshape, stride, pad):
    return torch.nn.grad.conv2d_weight(a, wshape, g, stride=stride, padding=pad)


def channel_stats(y):
    """per-channel mean and BIASED variance over (N, H, W), float64"""
    y = y.double()
    mean = y.mean(dim=(0, 2, 3))
    return mean, ((y - _bc(mean)) ** 2).mean(dim=(0, 2, 3))


def bnb_terms(g, x, k4, slope):
    """the three fused BatchNorm-backward reductions' TERMS for gradient g arriving at BatchNorm(x) (through a leaky activation when
    slope is given), k4 = [scale, shift, mean, invstd]: gg, gg * xhat per element (sum over N, H, W per channel) and g * z where
    z <= 0 (one sum over everything), float64; and what carries an error of g into them: |xhat|, |z| where z <= 0"""
    g, x, k4 = g.double(), x.double(), k4.double()
    z = _bc(k4[0]) * x + _bc(k4[1])
    neg = ~(z > 0) if slope is not None else torch.zeros_like(z, dtype=torch.bool)
    gg = torch.where(neg, float(torch.tensor(float(slope or 0.0), dtype=F32)) * g, g)
    xhat = (x - _bc(k4[2])) * _bc(k4[3])
    zero = torch.zeros_like(g)
    return NS(gg=gg, ggx=gg * xhat, gz=torch.where(neg, g * z, zero), xhat=xhat.abs(), zneg=torch.where(neg, z.abs(), zero))


# ---- exactness budget and bounds -----------------------------------------------------------------------------------------------------
def step_of(t):
    """the finest binary grid step that occurs in t: the largest power of two of which every value is an integer multiple"""
    t = t.double().reshape(-1)
    t = t[t != 0]
    if t.numel() == 0:
        return 1.0
    for e in range(8, -60, -1):
        s = t * 2.0 ** -e
        if bool((s == s.round()).all()):
            return 2.0 ** e
    raise ValueError('not on a binary grid')


def gamma(k):
    return k * U / (1 - k * U)


def half_ulp_bf16(v):
    """half a bf16 ulp at magnitude v (8 significand bits): 2^(floor(log2 v) - 8)"""
    v = v.double().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(v)) - 8)


def stats_bounds(y64, e_y, lane, merges, tiles_per_row):
    """Bounds of the merged per-channel mean and biased variance (the test merges the partial rows (count, mean, M2) in float64 with
    Chan's formula) for values y64 + (an error of at most e_y per element), from the arithmetic of the three forward epilogues:
      conv_bf16.hip / conv_deep.hip   a lane sums its `lane` values (a chain of `lane` additions), mu = sum * (1 / n), M2 = sum (y - mu)^2;
                                      the lane halves and the waves join by `merges` Chan merges  mu += dl * f, M2 += M2b + dl^2 n f
      conv_trunk.hip                  a lane keeps sum (y - shift) and sum (y - shift)^2 in two chains of 16 values per tile (shift =
                                      the mean of its first 16 values), mu = shift + s1 / n, M2 = s2 - s1 * (s1 / n); two Chan merges
    Mean.  A two-pass lane mean carries (lane + 2) roundings relative to the values' magnitude.  A merge is a convex combination of the
    two means (their errors do not add) plus the roundings of dl, f, dl * f and the sum: u (3 f |dl| + |mu|) <= 8 u max|y| per level
    (f <= 1; 4 u max|y| where both sides always hold the same count, f = 1 / 2: the trunk kernel's full tiles).  So, two-pass:
      e_mean = (lane + 2 + 8 merges) u R,  R = max|y| of the channel,
    and e_rms, the same with R = rms(y), bounds the count-weighted rms of the row means' errors (a lane's mean|y| <= its rms).
    The shifted form rounds relative to d = y - shift instead -- that is its point: |d| <= 2 max|y - mean| =: 2 Dmax, and a lane's
    rms(d) <= sqrt(1 + 2 T) sigma_lane (see (a)) -- and adds shift + s1 / n:
      e_mean = ((lane + 2) 2 Dmax + (2 + 4 merges) R) u,   e_rms = ((lane + 2) sqrt(1 + 2 T) sigma + (2 + 4 merges) rms(y)) u
    Variance.  (a) Inside a lane sum (y - mu_hat)^2 = M2 + n e^2 exactly -- the mean's error enters in second order -- and the chain
    rounds (lane + 4) times relative to M2 (all terms positive); a merge adds three roundings: (lane + 3 merges + 8) u var.  The
    shifted form rounds (lane + 6) times relative to s2 = sum (y - shift)^2 <= (1 + 2 T) M2_lane for T tiles per row (shift is the mean
    of 16 of the lane's 32 T values: (mean_16 - mean)^2 <= M2_lane / 16 by Cauchy-Schwarz): (lane + 6) (1 + 2 T) u var.  c1 = the larger.
    (b) The cross terms: 2 n_r e_r (mu_r - mean) of the rows sum to at most 2 e_rms sigma (Cauchy-Schwarz, sum n_r (mu_r - mean)^2 <=
    N var); the merges' 2 (e_a + e_b) |dl| w, w = n nb / nt <= min(n, nb): sum w dl^2 over ALL merges is the between-lane sum of
    squares <= N var, sum w <= N / 2 per level, (e_a + e_b)^2 <= 2 (e_a^2 + e_b^2): at most 2 sqrt(2 merges) e_rms sigma.
      e_var = c1 u var + (2 + 2 sqrt(2 merges)) e_rms sigma + e_mean^2
    The error e_y of the values themselves (tier B) adds mean(e_y) to the mean and 2 sigma rms(e_y) + mean(e_y^2) to the variance."""
    mean, var = channel_stats(y64)
    sigma = var.sqrt()
    r_max = y64.abs().amax(dim=(0, 2, 3))
    rms = (y64 ** 2).mean(dim=(0, 2, 3)).sqrt()
    if tiles_per_row:
        d_max = (y64 - _bc(mean)).abs().amax(dim=(0, 2, 3))
        e_mean = ((lane + 2) * 2 * d_max + (2 + 4 * merges) * r_max) * U
        e_rms = ((lane + 2) * math.sqrt(1 + 2 * tiles_per_row) * sigma + (2 + 4 * merges) * rms) * U
    else:
        e_mean, e_rms = (lane + 2 + 8 * merges) * U * r_max, (lane + 2 + 8 * merges) * U * rms
    c1 = max(lane + 3 * merges + 8, (lane + 6) * (1 + 2 * tiles_per_row) if tiles_per_row else 0)
    e_var = c1 * U * var + (2 + 2 * math.sqrt(2 * merges)) * e_rms * sigma + e_mean ** 2
    if e_y is not None:
        e_mean = e_mean + e_y.mean(dim=(0, 2, 3))
        e_var = e_var + 2 * sigma * (e_y ** 2).mean(dim=(0, 2, 3)).sqrt() + (e_y ** 2).mean(dim=(0, 2, 3))
    return NS(mean=mean, var=var, e_mean=e_mean, e_var=e_var, sigma=sigma)


# chain lengths, counted from the kernels: values per lane and channel, Chan merges, and for the plain sums of the
# BatchNorm-backward epilogue the longest chain of additions (lane chain + shuffle + waves) plus the roundings of a term itself
#   conv_bf16.hip   lane: 16 MSUB <= 32 rows; merges: lane halves + three waves in sequence = 4
#   conv_deep.hip   lane: 32 rows; merges: lane halves + two waves = 2
#   conv_trunk.hip  lane: two chains of 16 per tile, joined: 16 T + 1; merges: lane halves + two waves = 2
STAT_CHAIN = {'generic': (32, 4), 'deep': (32, 2)}


def stat_chain(family, tiles_per_row=1):
    if family == 'trunk':
        return 16 * tiles_per_row + 1, 2, tiles_per_row
    lane, merges = STAT_CHAIN[family]
    return lane, merges, 0


def bnb_depth(family, cout_tile=64, tiles_per_row=1):
    """longest chain of additions of a partial row of the fused reductions -> (per-channel sums, the slope sum); + 4: the roundings of
    a term (slope * g, x - mean, * invstd, the product; the trunk kernel's x * is - mean * is has as many)
      conv_bf16.hip / conv_deep.hip   32 lane values + shuffle + 3 (1) waves; slope sum: 32 values x the lane's cout sub-tiles
                                      (cout_tile / 32) in one chain + 6 butterfly levels + 3 waves
      conv_trunk.hip                  two chains of 16 T, joined, + shuffle + one wave pair; slope sum: the same chain + 6 + 2"""
    if family == 'trunk':
        lane = 16 * tiles_per_row + 1
        return lane + 2 + 4, lane + 8 + 4
    return 32 + 4 + 4, 32 * (cout_tile // 32) + 9 + 4


# ---- cases -------------------------------------------------------------------------------------------------------------------------
def _consts(pro, c, tier, seed, coarse):
    """the per-channel constants and the slope of prologue `pro` over c channels"""
    k = {}
    if tier == 'grid':
        if coarse:
            sl = 0.5
            if pro == AFFINE_ACT:
                k.update(pa=choice((c,), [0.5, 1.0], seed), pd=choice((c,), [-0.5, 0.0, 0.5], seed + 1))
            if pro in (BNBWD, BNACT_BWD):
                k.update(pa=choice((c,), [0.5, 1.0], seed), pb=choice((c,), [-0.5, 0.0, 0.5], seed + 1),
                         pd=choice((c,), [-0.25, 0.0, 0.25], seed + 2))
            if pro == BNACT_BWD:
                k.update(ps=choice((c,), [0.5, 1.0], seed + 3), pt=choice((c,), [-0.5, 0.0, 0.5], seed + 4))
        else:
            sl = 0.25
            if pro == AFFINE_ACT:
                k.update(pa=choice((c,), [0.5, 0.75, 1.0, 1.25, 1.5], seed), pd=grid((c,), 2.0 ** -4, 0.5, seed + 1))
            if pro in (BNBWD, BNACT_BWD):
                k.update(pa=choice((c,), [0.5, 1.0, 1.5], seed), pb=choice((c,), [-0.5, 0.0, 0.5], seed + 1),
                         pd=grid((c,), 2.0 ** -3, 0.5, seed + 2))
            if pro == BNACT_BWD:
                k.update(ps=choice((c,), [0.5, 1.0, 1.5], seed + 3), pt=grid((c,), 0.25, 1.0, seed + 4))
            if pro == RES_AFFINE:
                k.update(pa=choice((c,), [0.5, 1.0, 1.5], seed), pd=grid((c,), 2.0 ** -3, 0.5, seed + 1))
    else:
        sl = 0.2
        if pro in (AFFINE_ACT, RES_AFFINE):
            k.update(pa=rand((c,), seed) * 0.5 + 1.0, pd=rand((c,), seed + 1, 0.3))
        if pro in (BNBWD, BNACT_BWD):
            k.update(pa=rand((c,), seed) * 0.3 + 1.0, pb=rand((c,), seed + 1, 0.2), pd=rand((c,), seed + 2, 0.1))
        if pro == BNACT_BWD:
            k.update(ps=rand((c,), seed + 3) * 0.5 + 1.0, pt=rand((c,), seed + 4, 0.3))
    if pro in (ACT, AFFINE_ACT, BNACT_BWD, ACT_BWD, RES_AFFINE):
        k['slope'] = sl
    return k


def make_operand(pro, shape, tier, seed, coarse=False, rounded=True, no_slope=False):
    """seeded input tensors + constants of one lazy operand over `shape` = (n, c, h, w) -> (kwargs of operand(), the staged values).
    rounded: tier B values are made representable in bf16 (bf16 storage); False keeps ordinary fp32 values (SISR_STORAGE=f32 and the
    fp32 NCHW images).  Grid values are representable in both."""
    c = shape[1]
    k = _consts(pro, c, tier, seed + 10, coarse)
    if no_slope:                                           # RES_AFFINE without an activation on the residual
        k['slope'] = None
    fix = bf if rounded else (lambda t: t)
    two = pro in TWO_TENSOR
    if tier == 'grid':
        if coarse:
            k['x1'] = grid(shape, 0.5, 1.0, seed)
            if two:
                k['x2'] = grid(shape, 0.5, 1.0, seed + 1)
        elif not two:
            k['x1'] = grid(shape, 2.0 ** -4, 2.0, seed)
        else:
            k['x1'] = grid(shape, 2.0 ** -3, 1.0, seed)
            k['x2'] = grid(shape, 0.25, 1.0 if pro in (TANH_BWD, RES_AFFINE) else 2.0, seed + 1)
    else:
        k['x1'] = fix(rand(shape, seed, 1.0 if two and pro != RES_AFFINE else 2.0))
        if two:
            k['x2'] = fix(rand(shape, seed + 1, 1.0 if pro == TANH_BWD else 2.0))
    return k, operand(pro, **k)


def make_weights(cout, cin, k, tier, seed, coarse=False, bias=True):
    if tier == 'grid':
        w = grid((cout, cin, k, k), 2.0 ** -4 if coarse else 2.0 ** -6, 0.25, seed)
        b = grid((cout,), 2.0 ** -6, 0.5, seed + 1) if bias else None
    else:
        w = rand((cout, cin, k, k), seed, (1.0 / (cin * k * k)) ** 0.5 * 1.7)
        b = rand((cout,), seed + 1, 0.1) if bias else None
    return w, b


def make_bnb(shape, tier, seed, act):
    """the BatchNorm in front of a data gradient: its input x (bf16-representable), k4 = [scale, shift, mean, invstd], slope | None"""
    c = shape[1]
    if tier == 'grid':
        x = grid(shape, 0.25, 2.0, seed)
        k4 = torch.stack([choice((c,), [0.5, 1.0, 1.5], seed + 1), grid((c,), 0.25, 1.0, seed + 2), grid((c,), 0.25, 0.5, seed + 3),
                          choice((c,), [0.5, 1.0, 2.0], seed + 4)])
        return x, k4, (0.25 if act else None)
    x = bf(rand(shape, seed, 2.0))
    k4 = torch.stack([rand((c,), seed + 1) * 0.5 + 1.0, rand((c,), seed + 2, 0.3), rand((c,), seed + 3, 0.2), rand((c,), seed + 4) * 0.5 + 1.0])
    return x, k4, (0.2 if act else None)


@functools.lru_cache(maxsize=None)
def conv_case(role, geom, pro, tier, seed=0, res=False, bnb=None, coarse=False, rounded=True, out_bf16=True, bias=True, shuffle2=False,
              no_slope=False):
    """One forward ('fwd') or data-gradient ('dgrad') launch.  geom = (n, cin, cout, k, stride, h, w) of the FORWARD convolution; the
    data gradient contracts the gradient operand (n, cout, ho, wo) with the same weights.  bnb: None | 'plain' | 'act' (the fused
    BatchNorm-backward reductions of the result).  -> namespace: the operand's inputs `k` and staged values `op`, w, b, res,
    ref (float64, before the storage rounding of the output), bound (tier B: gamma_K S + A, + half a bf16 ulp when the output is
    stored as bf16; tier A: None), budget (largest S in grid steps), and for bnb the inputs and the three sums with their terms."""
    n, cin, cout, k, stride, h, w = geom
    pad = k // 2
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    wt, b = make_weights(cout, cin, k, tier, 1000 + seed, coarse, bias and role == 'fwd')
    wq = bf(wt).double()
    if role == 'fwd':
        kw, op = make_operand(pro, (n, cin, h, w), tier, 2000 + seed, coarse, rounded, no_slope)
        f = lambda a, ww, bb: conv_fwd(a, ww, bb, stride, pad)
        terms, oshape = cin * k * k, (n, cout, ho, wo)
    else:
        # (shuffle2: the gradient is the [n, cout / 4, 2 ho, 2 wo] tensor behind the PixelShuffle, read through the un-shuffling view)
        gshape = (n, cout // 4, 2 * ho, 2 * wo) if shuffle2 else (n, cout, ho, wo)
        kw, op = make_operand(pro, gshape, tier, 2000 + seed, coarse, rounded)
        view = (lambda a: F.pixel_unshuffle(a, 2)) if shuffle2 else (lambda a: a)
        f = lambda a, ww, bb: conv_dgrad(view(a), ww, stride, pad, (h, w))
        terms, oshape = cout * k * k, (n, cin, h, w)
    if shuffle2 and role == 'fwd':
        oshape = (n, cout // 4, 2 * ho, 2 * wo)
    b64 = None if b is None else b.double()
    post = pixel_shuffle2 if shuffle2 and role == 'fwd' else (lambda t: t)
    ref = post(f(op.q, wq, b64))
    s = post(f(op.q.abs(), wq.abs(), None if b is None else b64.abs()))
    r = None
    if res:
        r = grid(oshape, 2.0 ** -4, 2.0, 3000 + seed) if tier == 'grid' else bf(rand(oshape, 3000 + seed))
        ref, s = ref + r.double(), s + r.double().abs()
    assert tuple(ref.shape) == oshape
    out = NS(role=role, geom=geom, pro=pro, tier=tier, k=kw, op=op, w=wt, b=b, res=r, ref=ref, s=s, terms=terms, out_bf16=out_bf16,
             oshape=oshape, bound=None, budget=None, share=float(op.ambiguous.double().mean()))
    if tier == 'grid':
        steps = [step_of(op.q) * step_of(wq)] + [step_of(t) for t in (b, r) if t is not None]
        out.step = min(steps)
        out.budget = float(s.max()) / out.step
        out.stored = bf(ref) if out_bf16 else ref
    else:
        amb = post(f((op.alt - op.q).abs(), wq.abs(), None))
        out.bound = gamma(terms + 2) * s + amb
        out.e_acc = out.bound                      # the error of the fp32 value the epilogue holds (statistics, reductions)
        if out_bf16:
            out.bound = out.bound + half_ulp_bf16(ref.abs() + out.bound)
    if bnb is not None:
        assert role == 'dgrad'
        xb, k4, bslope = make_bnb(oshape, tier, 4000 + seed, bnb == 'act')
        out.bnb = NS(x=xb, k4=k4, slope=bslope, terms=bnb_terms(ref, xb, k4, bslope))
    return out


def bnb_reference(case, depth_c, depth_s):
    """sums and bounds of the fused reductions of a data-gradient case: (D + r) u sum |terms| for the chain depths given, plus (tier B)
    the error e_g of the gradient the epilogue holds, carried through each term (all three are linear in g, |gg| <= |g|)"""
    t = case.bnb.terms
    dims = (0, 2, 3)
    refs = [t.gg.sum(dims), t.ggx.sum(dims), t.gz.sum().reshape(1)]
    bounds = [depth_c * U * t.gg.abs().sum(dims), depth_c * U * t.ggx.abs().sum(dims), depth_s * U * t.gz.abs().sum().reshape(1)]
    if case.tier != 'grid':
        e = case.e_acc
        bounds[0] = bounds[0] + e.sum(dims)
        bounds[1] = bounds[1] + (e * t.xhat).sum(dims)
        bounds[2] = bounds[2] + (e * t.zneg).sum().reshape(1)
    return refs, bounds


@functools.lru_cache(maxsize=None)
def wgrad_case(geom, xpro, gpro, tier, seed=0, coarse=True, x_rounded=True, g_rounded=True, sparse=1.0, shuffle2=False):
    """One weight-gradient launch: dW = sum over pixels of x'(pixel + tap) (x) dy'(pixel), bias gradient = sum of the UN-ROUNDED dy'.
    sparse < 1: a seeded share of the gradient operand's pixels is zeroed on grid cases (keeps large shapes inside the budget).
    shuffle2: the gradient is the [n, cout / 4, 2 ho, 2 wo] tensor behind the PixelShuffle, read through the un-shuffling view."""
    n, cin, cout, k, stride, h, w = geom
    pad = k // 2
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    kx, xo = make_operand(xpro, (n, cin, h, w), tier, 5000 + seed, coarse, x_rounded)
    kg, go = make_operand(gpro, (n, cout // 4, 2 * ho, 2 * wo) if shuffle2 else (n, cout, ho, wo), tier, 6000 + seed, coarse, g_rounded)
    if sparse < 1.0:
        assert tier == 'grid' and gpro in (NONE, ACT_BWD, TANH_BWD)            # (prologues with f(0) = 0)
        keep = (torch.rand((n, 1, ho, wo), generator=_gen(6500 + seed)) < sparse).to(F32)
        kg['x1'] = kg['x1'] * keep
        go = operand(gpro, **kg)
    wshape = (cout, cin, k, k)
    if shuffle2:                                              # elementwise prologue first, then the view: original channel order 4 c + 2 i + j
        go = NS(**{name: F.pixel_unshuffle(getattr(go, name), 2) for name in ('v', 'q', 'alt', 'mag')}, ambiguous=go.ambiguous,
                evals=[F.pixel_unshuffle(e, 2) for e in go.evals])
    f = lambda a, g: conv_wgrad(a, g, wshape, stride, pad)
    ref = f(xo.q, go.q)
    s = f(xo.q.abs(), go.q.abs())
    dims = (0, 2, 3)
    pix = n * ho * wo
    out = NS(geom=geom, xpro=xpro, gpro=gpro, tier=tier, kx=kx, kg=kg, xo=xo, go=go, ref=ref, s=s, terms=pix,
             gb_ref=go.v.sum(dims), bound=None, budget=None,
             share=max(float(xo.ambiguous.double().mean()), float(go.ambiguous.double().mean())))
    if tier == 'grid':
        out.step = step_of(xo.q) * step_of(go.q)
        out.budget = max(float(s.max()) / out.step, float(go.v.abs().sum(dims).max()) / step_of(go.v))
    else:
        dx, dg = (xo.alt - xo.q).abs(), (go.alt - go.q).abs()
        amb = f(dx, go.q.abs()) + f(xo.q.abs(), dg) + f(dx, dg)
        out.bound = gamma(pix + 8) * s + amb
        # bias gradient: a sum of `pix` un-rounded fp32 values in some order (any order: gamma_pix), each within 5 roundings
        # (the prologue's operations, contracted or not) of the float64 value
        out.gb_bound = (pix + 5) * U * go.mag.sum(dims)
    return out


# ---- the case tables of tests/test_gpu_bf16_exact.py --------------------------------------------------------------------------------
# (n, cin, cout, k, stride, h, w)
GENERIC = [(2, 64, 64, 3, 1, 12, 12), (1, 64, 64, 3, 1, 37, 29), (2, 32, 128, 3, 1, 8, 8), (2, 128, 64, 3, 1, 6, 6),
           (2, 64, 128, 3, 2, 16, 16), (2, 64, 64, 1, 1, 12, 12)]
RAGGED = GENERIC[1]
# (n, h, w[, cap]): cap = SISR_PERSIST_MAX_WG.  tiles = n (h / 8) (w / 16); sisr_equal_shares: rounds = ceil(tiles / slots),
# workgroups = ceil(tiles / rounds) -> walks of 1 | 2 (one workgroup) | 2 + 1 (uneven) | 9 x 3 (across rows and images) | 8 x 1
TRUNK = [(1, 8, 16), (1, 16, 16, 1), (1, 24, 16, 2), (3, 24, 48, 10), (2, 16, 32)]
TRUNK_WALK = {(1, 8, 16): (1, 1), (1, 16, 16, 1): (1, 2), (1, 24, 16, 2): (2, 2), (3, 24, 48, 10): (9, 3), (2, 16, 32): (8, 1)}
WALK27 = TRUNK[3]
# (n, cin, cout, stride, h, w): the first seven SMALL cases of tests/test_gpu_deep.py + the K split
DEEP = [(3, 64, 64, 1, 12, 12), (5, 32, 128, 1, 6, 6), (2, 64, 128, 1, 24, 24), (2, 128, 64, 1, 16, 32), (2, 64, 64, 1, 37, 29),
        (3, 64, 128, 2, 24, 24), (2, 64, 64, 2, 32, 32), (4, 256, 512, 1, 12, 12)]
DEEP_WG = [(3, 64, 64, 1, 12, 12), (5, 64, 128, 1, 6, 6), (2, 64, 128, 1, 24, 24), (2, 128, 64, 1, 16, 32), (2, 64, 64, 1, 37, 29),
           (3, 64, 128, 2, 24, 24), (2, 64, 64, 2, 32, 32), (3, 64, 64, 2, 13, 11), (4, 256, 512, 1, 12, 12), (4, 512, 512, 2, 12, 12)]
THIN = [(1, 16, 16), (2, 16, 32), (3, 48, 48, 4)]
TOIMAGE = [(2, 16, 32), (3, 13, 31)]
WG_THIN = [(2, 16, 32), (3, 24, 64, 3)]
# (x prologue, gradient prologue).  wgrad_bf16.hip takes every pair.  wgrad_trunk.hip instantiates the gradient prologues BNBWD and
# BNACT_BWD only (and ACT_BWD for the upscale conv, Cout = 256 through the un-shuffling view: TRUNK_UP below), so its first pair is
# (NONE, BNBWD) where the generic kernel's is (NONE, NONE); wgrad_deep.hip keeps the four pairs tests/test_gpu_deep.py runs it with.
WG_PAIRS = [(NONE, NONE), (ACT, BNACT_BWD), (AFFINE_ACT, BNBWD), (AFFINE_ACT, BNACT_BWD)]
WG_TRUNK_PAIRS = [(NONE, BNBWD), (ACT, BNACT_BWD), (AFFINE_ACT, BNBWD), (AFFINE_ACT, BNACT_BWD)]
DEEP_WG_PAIRS = [(NONE, NONE), (ACT, ACT_BWD), (AFFINE_ACT, BNACT_BWD), (AFFINE_ACT, BNBWD)]
FWD_PROS = [NONE, ACT, AFFINE_ACT]


def trunk_geom(shape):
    return (shape[0], 64, 64, 3, 1, shape[1], shape[2])


def deep_geom(case):
    n, cin, cout, stride, h, w = case
    return (n, cin, cout, 3, stride, h, w)


def equal_shares(total, slots):
    rounds = -(-total // max(slots, 1))
    return -(-total // rounds), rounds


# ---- the launches of tests/test_gpu_bf16_exact.py, one tuple per parametrised case ------------------------------------------------------
# family: which kernel the launch must reach; shape: a generic geometry, a trunk (n, h, w[, cap]) or a deep case; storage: SISR_STORAGE
class ConvRun(NS):
    def __repr__(self):
        return '-'.join(str(v).replace(' ', '') for v in (self.family, self.role, self.shape, PRO_NAMES[self.pro], self.tier, self.storage,
                                                          'res' if self.res else '', self.bnb or '', 'shuffle' if self.shuffle2 else '',
                                                          self.tag) if v != '')


PRO_NAMES = ['none', 'act', 'affine_act', 'bnbwd', 'bnact_bwd', 'act_bwd', 'tanh_bwd', 'res_affine']
UPSCALE = (2, 64, 256, 3, 1, 12, 12)
LAST_CONV = (3, 64, 3, 3, 1, 13, 31)


def _run(family, role, shape, pro, tier, storage='bf16', res=False, bnb=None, shuffle2=False, coarse=False, tag='', **kw):
    return ConvRun(family=family, role=role, shape=shape, pro=pro, tier=tier, storage=storage, res=res, bnb=bnb, shuffle2=shuffle2,
                   coarse=coarse, tag=tag, **kw)


DG_COMBOS = [(NONE, False, None), (BNBWD, True, 'plain'), (BNACT_BWD, True, 'act'), (ACT_BWD, False, 'act'), (BNACT_BWD, False, None)]
DG_REST = [(NONE, True, 'plain'), (BNBWD, False, 'act'), (ACT_BWD, True, None)]
TRUNK_DG_COMBOS = [(BNBWD, False, None), (BNBWD, True, 'plain'), (BNACT_BWD, True, 'act'), (BNACT_BWD, False, 'plain')]


def _conv_runs():
    r = []
    for st in ('bf16', 'f32'):
        for g in GENERIC:
            r += [_run('generic', 'fwd', g, pro, 'grid', st) for pro in FWD_PROS]
            r += [_run('generic', 'dgrad', g, pro, 'grid', st, res, bnb) for pro, res, bnb in DG_COMBOS]
        r.append(_run('generic', 'fwd', UPSCALE, ACT, 'grid', st, shuffle2=True))
        r += [_run('generic', 'dgrad', UPSCALE, ACT_BWD, 'grid', st, res, shuffle2=True) for res in (False, True)]
        # the generator's last conv kept on the generic kernel (SISR_THIN=0): NCHW fp32 image, tanh epilogue off / on
        r += [_run('generic', 'fwd', LAST_CONV, ACT, 'grid', st, tag=t) for t in ('nchw', 'tanh')]
        r += [_run('generic', 'fwd', RAGGED, pro, 'rand', st) for pro in FWD_PROS]
        r += [_run('generic', 'dgrad', RAGGED, pro, 'rand', st, res, bnb) for pro, res, bnb in DG_COMBOS[1:3]]
    for sh in TRUNK:
        r += [_run('trunk', 'fwd', sh, pro, 'grid') for pro in FWD_PROS]
        r += [_run('trunk', 'fwd', sh, RES_AFFINE, 'grid', tag=t) for t in ('slope', 'noslope')]
        r += [_run('trunk', 'dgrad', sh, pro, 'grid', 'bf16', res, bnb) for pro, res, bnb in TRUNK_DG_COMBOS]
        # (the upscale conv: its data gradient reads 256 channels and stays with the generic kernel: UPSCALE above)
        r += [_run('trunk', 'fwd', sh, pro, 'grid', shuffle2=True) for pro in (NONE, ACT)]
    r += [_run('trunk', 'fwd', WALK27, pro, 'rand') for pro in FWD_PROS + [RES_AFFINE]]
    r += [_run('trunk', 'dgrad', WALK27, pro, 'rand', 'bf16', res, bnb) for pro, res, bnb in TRUNK_DG_COMBOS[1:3]]
    for c in DEEP:
        coarse = c[1] >= 256                                  # the K split: 2304 terms per element
        r += [_run('deep', 'fwd', c, pro, 'grid', coarse=coarse) for pro in FWD_PROS]
        r += [_run('deep', 'dgrad', c, pro, 'grid', 'bf16', res, 'act', coarse=coarse)
              for pro, res in ((NONE, False), (ACT_BWD, True), (BNACT_BWD, False))]
    r += [_run('deep', 'fwd', DEEP[5], AFFINE_ACT, 'rand'), _run('deep', 'dgrad', DEEP[5], BNACT_BWD, 'rand', 'bf16', True, 'act')]
    for sh in THIN:
        r += [_run('thin', 'fwd', sh, NONE, 'grid'), _run('thin', 'dgrad', sh, TANH_BWD, 'grid')]
    r += [_run('thin', 'fwd', THIN[1], NONE, 'rand'), _run('thin', 'dgrad', THIN[1], TANH_BWD, 'rand')]
    for sh in TOIMAGE:
        r += [_run('toimage', 'fwd', sh, pro, 'grid', tag=t) for pro in (NONE, ACT) for t in ('', 'tanh')]
    r += [_run('toimage', 'fwd', TOIMAGE[1], ACT, 'rand', tag=t) for t in ('', 'tanh')]
    # the rest of the generic data gradient's cross {NONE, BNBWD, BNACT_BWD, ACT_BWD} x {no residual, residual} (DG_COMBOS holds 5 of 8)
    for st in ('bf16', 'f32'):
        for g in GENERIC:
            r += [_run('generic', 'dgrad', g, pro, 'grid', st, res, bnb) for pro, res, bnb in DG_REST]
    for i, x in enumerate(r):
        x.seed = 7 * i
    return r


def run_geom(r):
    """the forward convolution's geometry (n, cin, cout, k, stride, h, w) of a run"""
    sh = r.shape
    if r.family == 'generic':
        return sh
    if r.family == 'deep':
        return deep_geom(sh)
    n, h, w = sh[:3]
    if r.family == 'trunk':
        return (n, 64, 256 if r.shuffle2 else 64, 3, 1, h, w)
    if r.family == 'thin':
        return (n, 3, 64, 9, 1, h, w) if r.role == 'fwd' else (n, 64, 3, 3, 1, h, w)
    return (n, 64, 3, 3, 1, h, w)                          # toimage


def image_out_run(r):
    """the output is the fp32 NCHW image"""
    return r.family == 'toimage' or r.tag in ('nchw', 'tanh')


def run_case(r):
    image_in = r.family == 'thin'                         # the operand is the fp32 NCHW image (or its gradient): ordinary fp32 values
    image_out = image_out_run(r)
    return conv_case(r.role, run_geom(r), r.pro, r.tier, seed=r.seed, res=r.res, bnb=r.bnb, coarse=r.coarse,
                     rounded=(r.storage == 'bf16' and not image_in), out_bf16=(r.storage == 'bf16' and not image_out),
                     bias=not (r.family == 'thin' and r.role == 'dgrad'), shuffle2=r.shuffle2, no_slope=r.tag == 'noslope')


CONV_RUNS = _conv_runs()


def stat_runs():
    """the forward runs whose launch also writes BatchNorm statistics rows (the thin / to-image kernels and the PixelShuffle store
    have no such epilogue)"""
    return [r for r in CONV_RUNS if r.role == 'fwd' and r.family in ('generic', 'trunk', 'deep') and not r.shuffle2 and not image_out_run(r)]


def run_stat_chain(r):
    if r.family == 'trunk':
        return stat_chain('trunk', TRUNK_WALK[r.shape][1])
    return stat_chain(r.family)


class WgRun(NS):
    def __repr__(self):
        return '-'.join(str(v).replace(' ', '') for v in (self.family, self.shape, PRO_NAMES[self.xpro], PRO_NAMES[self.gpro], self.tier,
                                                          self.storage, self.tag) if v != '')


TRUNK_UP = [(1, 16, 16, 1), (2, 16, 32), (3, 24, 48, 10)]
PADDED = (2, 64, 3, 3, 1, 20, 24)                 # test_wgrad_bf16_few_channel_output_padded's: not a to-image size (20 % 8)


def _wg_runs():
    r = []
    mk = lambda family, shape, xp, gp, tier, storage='bf16', tag='': WgRun(family=family, shape=shape, xpro=xp, gpro=gp, tier=tier,
                                                                         storage=storage, tag=tag)
    for st in ('bf16', 'f32'):
        for g in GENERIC:
            r += [mk('generic', g, xp, gp, 'grid', st) for xp, gp in WG_PAIRS]
        r.append(mk('generic', RAGGED, AFFINE_ACT, BNACT_BWD, 'rand', st))
    r.append(mk('generic', PADDED, NONE, TANH_BWD, 'grid', tag='padded'))
    for sh in TRUNK:
        r += [mk('trunk', sh, xp, gp, 'grid') for xp, gp in WG_TRUNK_PAIRS]
    r.append(mk('trunk', WALK27, AFFINE_ACT, BNACT_BWD, 'rand'))
    for c in DEEP_WG:
        r += [mk('deep', c, xp, gp, 'grid') for xp, gp in DEEP_WG_PAIRS]
    r.append(mk('deep', DEEP_WG[5], AFFINE_ACT, BNACT_BWD, 'rand'))
    for sh in WG_THIN:
        r += [mk('thin', sh, NONE, gp, 'grid', tag=t) for gp in (NONE, ACT_BWD) for t in ('k9', 'k3')]
        r += [mk('toimage', sh, xp, gp, 'grid') for xp, gp in ((NONE, NONE), (ACT, TANH_BWD))]
    r += [mk('thin', WG_THIN[0], NONE, ACT_BWD, 'rand', tag='k9'), mk('toimage', WG_THIN[0], ACT, TANH_BWD, 'rand')]
    # (appended: the seeds of the runs in front stay what they were) the other half of wgrad_toimage.hip's 2 x 2, and the trunk
    # kernel's ACT_BWD instance: the upscale conv, Cout = 256, gradient behind the PixelShuffle
    for sh in WG_THIN:
        r += [mk('toimage', sh, xp, gp, 'grid') for xp, gp in ((NONE, TANH_BWD), (ACT, NONE))]
    r += [mk('trunk', sh, ACT, ACT_BWD, 'grid', tag='up') for sh in TRUNK_UP]
    r.append(mk('trunk', TRUNK_UP[2], ACT, ACT_BWD, 'rand', tag='up'))
    for i, x in enumerate(r):
        x.seed = 11 * i
    return r


def wg_geom(r):
    sh = r.shape
    if r.family == 'generic':
        return sh
    if r.family == 'deep':
        return deep_geom(sh)
    n, h, w = sh[:3]
    if r.family == 'trunk':
        return (n, 64, 256 if r.tag == 'up' else 64, 3, 1, h, w)
    if r.family == 'thin':
        return (n, 3, 64, 9 if r.tag == 'k9' else 3, 1, h, w)
    return (n, 64, 3, 3, 1, h, w)


def wg_case(r):
    bf16 = r.storage == 'bf16'
    image_g = r.family == 'toimage' or r.tag == 'padded'      # the gradient is the fp32 NCHW image gradient
    return wgrad_case(wg_geom(r), r.xpro, r.gpro, r.tier, seed=r.seed, coarse=True, x_rounded=bf16 and r.family != 'thin',
                      g_rounded=bf16 and not image_g, shuffle2=r.tag == 'up')


WG_RUNS = _wg_runs()
# several layers in one launch: three members each
TRUNK_BATCH = [WgRun(family='trunk', shape=(2, 16, 32), xpro=AFFINE_ACT, gpro=BNBWD, tier='grid', storage='bf16', tag='batch', seed=9000 + i)
               for i in range(3)]
DEEP_BATCH = {1: [WgRun(family='deep', shape=c, xpro=AFFINE_ACT, gpro=BNACT_BWD, tier='grid', storage='bf16', tag='batch', seed=9100 + i)
                  for i, c in enumerate([DEEP_WG[0], DEEP_WG[2], DEEP_WG[4]])],
              2: [WgRun(family='deep', shape=c, xpro=AFFINE_ACT, gpro=BNACT_BWD, tier='grid', storage='bf16', tag='batch', seed=9200 + i)
                  for i, c in enumerate([DEEP_WG[5], DEEP_WG[6], DEEP_WG[7]])]}
# the default bf16 slabs against the fp32 slabs of the same launch (persistent trunk kernel, wgrad_deep.hip)
SLAB_RUNS = [r for r in WG_RUNS if r.tier == 'grid' and ((r.family == 'trunk' and (r.xpro, r.gpro) == (AFFINE_ACT, BNACT_BWD)) or
                                                         (r.family == 'deep' and (r.xpro, r.gpro) == (AFFINE_ACT, BNACT_BWD)
                                                          and r.shape in (DEEP_WG[0], DEEP_WG[4], DEEP_WG[5], DEEP_WG[8])))]


def all_wg_runs():
    return WG_RUNS + TRUNK_BATCH + DEEP_BATCH[1] + DEEP_BATCH[2]
