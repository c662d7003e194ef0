"""Seeded inputs, float64 references, the exactness budget and the derived bounds of the discriminator's classifier head
(csrc/fc_head.hip: sisr_fc_head_forward, sisr_fc_head_backward, sisr_fc1_dgrad, sisr_fc_wgrad_rows) -- everything of
tests/test_gpu_fc_head.py that needs no device, so that tests/test_fc_head_cases_cpu.py can check the conditions that keep the GPU
file from hiding a failure where there is no GPU.  Plain torch on the CPU.

All products of this family are exact fp32 (v_mfma_f32_16x16x4_f32, v_mfma_f32_32x32x2_f32) and every sum is fp32 in a fixed order.

Two tiers (the method of tests/bf16_cases.py).
  A, grid operands: every operand on a coarse binary grid, so every partial sum of every order is an integer multiple of the
     product of the grid steps and stays below 2^22 of them (budget()): the fp32 result equals the float64 reference bit for bit.
     Only this separates "one K step lost" from rounding: the rounding bound K u S is about one term once K is a few thousand.
  B, ordinary random fp32 operands, element by element:  |got - ref64| <= 2 gamma_D S,  gamma_D = D u / (1 - D u), S = the sum of the
     magnitudes of the element's terms, D = the longest chain of fp32 roundings the element passes through, counted from the kernel
     beside each depth_*() below (u = 2^-24).

The K slicing of fc1_forward_kernel: K / 16 steps of 16 floats are cut into 16 wave slices [steps sl / 16, steps (sl + 1) / 16); a
slice runs floor(len / 8) trips of the loop unrolled by FH_UNROLL = 8 (non-temporal loads) and len % 8 steps of the tail loop (plain
loads).  slices() restates that formula; the forward shapes are chosen by what it gives (tests/test_fc_head_cases_cpu.py asserts it)."""
import functools
from types import SimpleNamespace as NS

import torch

from bf16_cases import BUDGET, F32, U, choice, gamma, grid, rand                  # noqa: F401  (BUDGET, U: re-exported)

FH_B, FH_KQ, FH_UNROLL = 16, 4, 8                     # csrc/fc_head.hip
NSL = FH_KQ * 4                                       # wave slices of K
FR_MAXROWS, FR_CHUNK = 256, 64

# (B, K, N)
FORWARD = [(1, 16, 16),            # one step in all: tail loop only, 15 empty slices
           (3, 64, 128),           # the smallest shape engine.fc_head_ok admits: four slices of one step, twelve empty
           (15, 2048, 144),        # 8 steps per slice: the unrolled loop only; N a multiple of 16 only
           (16, 2816, 128),        # 11 steps per slice = 8 unrolled + 3 tail
           (5, 2880, 384),         # 180 steps: slices of 11 and 12; N = 384: a partial 256-stride trip of the finish kernel
           (16, 4160, 256)]        # 260 steps: slices of 16 (unrolled only) and 17 (16 + 1 tail) side by side; N = one full trip
# (B, N): one thread per hidden unit, workgroups of 256 -- one partial workgroup, half a workgroup, one full, 1.5, 1 + 16
BACKWARD = [(1, 16), (16, 128), (7, 256), (5, 384), (16, 272)]
# (B, K, N): a wave takes N / 4 weight rows in trips of 32 -- 1, 1, 3 and 9 trips
DGRAD = [(1, 64, 128), (16, 64, 128), (5, 192, 384), (13, 128, 1152)]
# (rows, K, N): 64 rows are staged per round and paired two at a time
ROWS = [(1, 128, 64), (2, 128, 64), (63, 128, 64), (64, 256, 64), (65, 128, 128), (129, 128, 64), (255, 256, 128), (256, 128, 64)]
SCALES = [1.0, 0.125]
# the head path against the generic path the discriminator falls back to (discriminator_engine.run_forward / run_backward)
TWO_PATHS = [(5, 192, 128), (16, 2880, 384)]
TIERS = ['grid', 'rand']


def slices(K):
    """lengths, in K steps of 16 floats, of the 16 wave slices of fc1_forward_kernel (sl = 4 kq + wave)"""
    steps = K >> 4
    return [steps * (sl + 1) // NSL - steps * sl // NSL for sl in range(NSL)]


def slice_ends(K):
    """one past the last K step of each wave slice"""
    steps = K >> 4
    return [steps * (sl + 1) // NSL for sl in range(NSL)]


def bnd(depth, s):
    return 2 * gamma(depth) * s


def lrelu(v, slope):
    return torch.where(v > 0, v, v * slope)


def f32(v):
    """a python float as the kernel receives it"""
    return float(torch.tensor(float(v), dtype=F32))


# ---- chain lengths, counted from csrc/fc_head.hip ------------------------------------------------------------------------------------
def depth_h1(K):
    """fc1_forward_kernel + fc_head_finish_kernel: a wave's accumulator takes the 16 terms of each K step of its slice (4 MFMAs of 4
    products: at most one rounding per product added), the longest slice has ceil(steps / 16) steps; the 4 waves of a workgroup are
    added in LDS (3), the 4 K quarters are added onto 0 in the finish kernel (4), then the bias (1)"""
    steps = K >> 4
    return 16 * ((steps + NSL - 1) // NSL) + 3 + 4 + 1


def depth_t(N):
    """fc_head_finish_kernel's second layer: a thread adds ceil(N / 256) terms, each with the roundings of slope * v and of the
    product (2); wave_sum 6 levels; block_sum adds the 4 wave totals onto 0 (4); the bias (1)"""
    return (N + 255) // 256 + 2 + 6 + 4 + 1


SIGMOID_ULPS = 8        # expf, 1 + e and the division at one ulp (2^-23) each of a result <= 1, rounded up (tests/test_gpu_glue.py)
D_D2 = 3                # fc_head_bwd_kernel: d2 = g * o * (1 - o): two products and the difference, each a relative rounding
D_D1 = D_D2 + 2         # d1 = d2 * w * (1 | slope)


def depth_bwd_sum(B, term):
    """fc_head_bwd_kernel's sums over the batch rows: a chain of B additions of terms that carry `term` roundings"""
    return B + term


def depth_dgrad(N):
    """fc1_dgrad_kernel: a wave contracts its N / 4 weight rows into one accumulator (4 per MFMA), the 4 waves are added in LDS (3)"""
    return N // 4 + 3


def depth_rows(rows):
    """fc_wgrad_rows_kernel: one accumulator takes every row (2 per MFMA; an odd count adds an exact zero), then * scale (1)"""
    return rows + 1


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
def _zeros_mixed(t, seed):
    """a fixed share of exact zeros of both signs: an eighth +0.0, an eighth -0.0"""
    r = torch.rand(t.shape, generator=torch.Generator().manual_seed(seed))
    t = t.clone()
    t[r < 0.125] = 0.0
    t[(r >= 0.125) & (r < 0.25)] = -0.0
    return t


@functools.lru_cache(maxsize=None)
def forward_case(shape, tier, seed=0):
    """x [B][K], W1 [N][K], b1 [N], W2 [N], b2 [1], slope.  Grid: x on 2^-3 in [-1, 1], W1 on 2^-4 in [-1, 1], b1 on 2^-2 in [-2, 2]:
    h1 lives on 2^-7.  W2 is a 2^-3 grid scaled by 2^-8 so that the pre-sigmoid sum stays where the sigmoid has a slope."""
    B, K, N = shape
    s = 100 + seed
    if tier == 'grid':
        c = NS(x=grid((B, K), 2.0 ** -3, 1.0, s), w1=grid((N, K), 2.0 ** -4, 1.0, s + 1), b1=grid((N,), 2.0 ** -2, 2.0, s + 2),
               w2=grid((N,), 2.0 ** -3, 1.0, s + 3) * 2.0 ** -8, b2=torch.tensor([0.375]), slope=0.25, step=2.0 ** -7)
    else:
        c = NS(x=rand((B, K), s), w1=rand((N, K), s + 1, K ** -0.5 * 1.7), b1=rand((N,), s + 2, 0.1),
               w2=rand((N,), s + 3, N ** -0.5 * 3), b2=torch.tensor([0.3]), slope=0.2, step=None)
    c.shape, c.tier = shape, tier
    return c


def forward_ref(c, with_b1=True, with_b2=True, x=None, w1=None):
    """-> h1 [B][N], y [B] in float64 with the sums of magnitudes; tier B: bound_h and bound_y (tier A: bound_h None, bound_y the
    second layer's roundings alone, h1 being exact).  y = sigmoid(t), t = lrelu(h1) . W2 + b2: an error e of h1 reaches t as at
    most sum |W2| e (slope <= 1), the sum itself rounds depth_t(N) deep, |sigmoid'| <= 1/4."""
    B, K, N = c.shape
    x = (c.x if x is None else x).double()
    w1 = (c.w1 if w1 is None else w1).double()
    w2, slope = c.w2.double(), f32(c.slope)
    h1, s_h = x @ w1.t(), x.abs() @ w1.abs().t()
    if with_b1:
        h1, s_h = h1 + c.b1.double(), s_h + c.b1.double().abs()
    r = NS(h1=h1, s_h=s_h, bound_h=None if c.tier == 'grid' else bnd(depth_h1(K), s_h))
    r.y, r.bound_y = second_layer(h1, r.bound_h, w2, c.b2.double() if with_b2 else None, slope)
    return r


def second_layer(h1, e_h, w2, b2, slope, depth=None):
    """y = sigmoid(lrelu(h1) . w2 + b2) and its bound for an h1 that carries an error of at most e_h (None: exact)"""
    N = h1.shape[1]
    a = lrelu(h1, slope)
    t, s_t = a @ w2, a.abs() @ w2.abs()
    if b2 is not None:
        t, s_t = t + b2, s_t + b2.abs()
    e_t = bnd(depth_t(N) if depth is None else depth, s_t)
    if e_h is not None:
        e_t = e_t + e_h @ w2.abs()
    return torch.sigmoid(t), 0.25 * e_t + SIGMOID_ULPS * U


@functools.lru_cache(maxsize=None)
def backward_case(shape, tier, seed=0):
    """g [B], y [B], h1 [B][N], W2 [N], slope: the inputs the C ABI takes.  Grid: y in {1/4, 1/2, 3/4}, g on 2^-2 (never 0), W2 on
    2^-3, slope 1/4, h1 on 2^-3 with an eighth +0.0 and an eighth -0.0: d2 lives on 2^-6, dW2 and d1 on 2^-11."""
    B, N = shape
    s = 200 + seed
    if tier == 'grid':
        g = grid((B,), 0.25, 2.0, s)
        g[g == 0] = 0.25
        c = NS(g=g, y=choice((B,), [0.25, 0.5, 0.75], s + 1), h1=_zeros_mixed(grid((B, N), 2.0 ** -3, 2.0, s + 2), s + 3),
               w2=grid((N,), 2.0 ** -3, 1.0, s + 4), slope=0.25, step=2.0 ** -11)
    else:
        c = NS(g=rand((B,), s), y=torch.sigmoid(rand((B,), s + 1, 3.0)), h1=_zeros_mixed(rand((B, N), s + 2), s + 3),
               w2=rand((N,), s + 4, N ** -0.5 * 3), slope=0.2, step=None)
    c.shape, c.tier = shape, tier
    return c


def backward_ref(c, g=None, y=None, h1=None, zero_gate=None):
    """-> float64 d1 [B][N], dW2 [N], db2 [1], db1 [N], each with its sum of magnitudes `s_*` and (tier B) `bound_*`.
    LeakyReLU' is the slope where h1 == 0 (either sign), as in torch; zero_gate: the value used there instead (a mutation)."""
    B, N = c.h1.shape
    g, y, h1 = ((d if v is None else v).double() for v, d in ((g, c.g), (y, c.y), (h1, c.h1)))
    w2, slope = c.w2.double(), f32(c.slope)
    d2 = g * y * (1 - y)
    gate = torch.where(h1 > 0, torch.ones_like(h1), torch.full_like(h1, slope))
    if zero_gate is not None:
        gate = torch.where(h1 == 0, float(zero_gate), gate)
    a = lrelu(h1, slope)
    d1 = d2[:, None] * w2[None, :] * gate
    r = NS(d2=d2, d1=d1, s_d1=d1.abs(), dW2=d2 @ a, s_dW2=d2.abs() @ a.abs(), db2=d2.sum().reshape(1), s_db2=d2.abs().sum().reshape(1),
           db1=d1.sum(0), s_db1=d1.abs().sum(0))
    if c.tier != 'grid':
        # d1: its own roundings.  dW2: a chain of B terms d2 * lrelu(h) (d2's 3 roundings, slope * h, the product).  db2: B terms d2.
        # db1: B terms d1.
        r.bound_d1 = bnd(D_D1, r.s_d1)
        r.bound_dW2 = bnd(depth_bwd_sum(B, D_D2 + 2), r.s_dW2)
        r.bound_db2 = bnd(depth_bwd_sum(B, D_D2), r.s_db2)
        r.bound_db1 = bnd(depth_bwd_sum(B, D_D1), r.s_db1)
    return r


@functools.lru_cache(maxsize=None)
def dgrad_case(shape, tier, seed=0):
    """d1 [B][N], W1 [N][K] -> dx [B][K] = d1 W1.  Grid: both on 2^-4 in [-1, 1]: dx lives on 2^-8."""
    B, K, N = shape
    s = 300 + seed
    if tier == 'grid':
        c = NS(d1=grid((B, N), 2.0 ** -4, 1.0, s), w1=grid((N, K), 2.0 ** -4, 1.0, s + 1), step=2.0 ** -8)
    else:
        c = NS(d1=rand((B, N), s), w1=rand((N, K), s + 1, K ** -0.5 * 1.7), step=None)
    c.shape, c.tier = shape, tier
    return c


def dgrad_ref(c, d1=None, w1=None):
    d1 = (c.d1 if d1 is None else d1).double()
    w1 = (c.w1 if w1 is None else w1).double()
    r = NS(dx=d1 @ w1, s=d1.abs() @ w1.abs())
    r.bound = None if c.tier == 'grid' else bnd(depth_dgrad(d1.shape[1]), r.s)
    return r


@functools.lru_cache(maxsize=None)
def rows_case(shape, tier, seed=0):
    """dy [rows][N], x [rows][K] -> dW [N][K] = scale dy^T x.  Grid: dy on 2^-4, x on 2^-3 in [-1, 1]: dW lives on 2^-7 scale."""
    rows, K, N = shape
    s = 400 + seed
    if tier == 'grid':
        c = NS(dy=grid((rows, N), 2.0 ** -4, 1.0, s), x=grid((rows, K), 2.0 ** -3, 1.0, s + 1), step=2.0 ** -7)
    else:
        c = NS(dy=rand((rows, N), s), x=rand((rows, K), s + 1), step=None)
    c.shape, c.tier = shape, tier
    return c


def rows_ref(c, scale=1.0, rows=None):
    """rows: contract the first `rows` rows only (a mutation)"""
    dy, x = c.dy.double()[:rows], c.x.double()[:rows]
    r = NS(dW=(dy.t() @ x) * scale, s=(dy.abs().t() @ x.abs()) * scale)
    r.bound = None if c.tier == 'grid' else bnd(depth_rows(c.shape[0]), r.s)
    return r


@functools.lru_cache(maxsize=None)
def two_path_case(shape, tier):
    """the forward case of `shape` plus what the backward needs: g [B] for the chain (tier B), and a d1 [B][N] on the 2^-4 grid for
    the exact comparisons of dx = d1 W1 and dW1 = d1^T x (tier A: a d1 that comes from the sigmoid is on no grid)"""
    B, K, N = shape
    c = forward_case(shape, tier)
    return NS(fwd=c, shape=shape, tier=tier, g=rand((B,), 551), d1=grid((B, N), 2.0 ** -4, 1.0, 552) if tier == 'grid' else rand((B, N), 552))


def wgrad_ref(d1, x):
    d1, x = d1.double(), x.double()
    return d1.t() @ x, d1.abs().t() @ x.abs()


# ---- the exactness budget ------------------------------------------------------------------------------------------------------------
def budget(kind, case):
    """the worst sum of magnitudes of a tier-A case in steps of its finest grid (the result grid of its finest output)"""
    assert case.tier == 'grid'
    if kind == 'forward':
        return float(forward_ref(case).s_h.max()) / case.step
    if kind == 'backward':
        r = backward_ref(case)
        return max(float(t.max()) for t in (r.s_d1, r.s_dW2, r.s_db2, r.s_db1)) / case.step
    if kind == 'dgrad':
        return float(dgrad_ref(case).s.max()) / case.step
    if kind == 'rows':
        return float(rows_ref(case).s.max()) / case.step
    if kind == 'two_path':
        f = case.fwd
        return max(float(forward_ref(f).s_h.max()) / f.step, float((case.d1.double().abs() @ f.w1.double().abs()).max()) / 2.0 ** -8,
                   float(wgrad_ref(case.d1, f.x)[1].max()) / 2.0 ** -7)
    raise ValueError(kind)


def representable(t):
    """a float64 tensor that fp32 holds exactly"""
    return torch.equal(t.float().double(), t)
