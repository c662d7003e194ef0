"""CPU: the conditions on the seeded cases of tests/test_gpu_bf16_exact.py (tests/bf16_cases.py) that keep that file from hiding a
failure -- every grid case inside the 2^22 exactness budget, its operands after the prologue exact in bf16 and its fp32 CPU
contraction bit-equal to the float64 one; every random case with at most 0.1 % ambiguous operand values and an fp32 CPU evaluation
that passes the bound the case sets for the kernel; the derived statistics bounds fine enough to mean something; and the operand
builders against oracle/ops.py where that module restates the same operation."""
import pytest
import torch

import bf16_cases as B
from oracle import ops

CONV_GRID = [r for r in B.CONV_RUNS if r.tier == 'grid']
CONV_RAND = [r for r in B.CONV_RUNS if r.tier == 'rand']
WG_GRID = [r for r in B.all_wg_runs() if r.tier == 'grid']
WG_RAND = [r for r in B.all_wg_runs() if r.tier == 'rand']


def _f32_conv(c, a32, w32):
    """the case's contraction evaluated by torch in fp32 on the staged operands"""
    n, cin, cout, k, stride, h, w = c.geom
    b32 = None if c.b is None else c.b
    if c.role == 'fwd':
        y = B.conv_fwd(a32, w32, b32, stride, k // 2)
        y = B.pixel_shuffle2(y) if tuple(y.shape) != c.oshape else y
    else:
        g = torch.nn.functional.pixel_unshuffle(a32, 2) if a32.shape[1] != cout else a32
        y = B.conv_dgrad(g, w32, stride, k // 2, (h, w))
    return y if c.res is None else y + c.res


@pytest.mark.parametrize('run', CONV_GRID, ids=repr)
def test_grid_conv_case_is_exact(run):
    c = B.run_case(run)
    assert c.budget < B.BUDGET, c.budget
    assert c.share == 0.0 and torch.equal(c.op.alt, c.op.q)
    for t in (c.op.v, c.w.double()) + (() if c.res is None else (c.res.double(),)):
        assert torch.equal(B.bf(t), t), 'an operand is not representable in bf16'
    assert torch.equal(c.op.q, c.op.v)
    y32 = _f32_conv(c, c.op.q.float(), c.w)
    assert y32.dtype == torch.float32 and torch.equal(y32.double(), c.ref), 'fp32 and float64 CPU convolutions differ'
    if run.bnb:
        for t in (c.bnb.x, c.bnb.k4):
            assert torch.equal(B.bf(t), t)


@pytest.mark.parametrize('run', WG_GRID, ids=repr)
def test_grid_weight_gradient_case_is_exact(run):
    c = B.wg_case(run)
    assert c.budget < B.BUDGET, c.budget
    assert c.share == 0.0
    for o in (c.xo, c.go):
        assert torch.equal(B.bf(o.v), o.v) and torch.equal(o.q, o.v)
    n, cin, cout, k, stride, h, w = c.geom
    g32 = B.conv_wgrad(c.xo.q.float(), c.go.q.float(), (cout, cin, k, k), stride, k // 2)
    assert g32.dtype == torch.float32 and torch.equal(g32.double(), c.ref)
    assert torch.equal(c.go.v.float().sum(dim=(0, 2, 3)).double(), c.gb_ref)


@pytest.mark.parametrize('run', CONV_RAND, ids=repr)
def test_random_conv_case_reference_passes_its_own_bound(run):
    c = B.run_case(run)
    assert c.share <= 1e-3, c.share
    if run.storage == 'f32' or run.family == 'thin':
        x = c.k['x1']
        assert not torch.equal(B.bf(x), x), 'fp32-storage inputs must not be bf16-representable'
    y = _f32_conv(c, c.op.q.float(), B.bf(c.w))
    y = B.bf(y) if c.out_bf16 else y
    err = (y.double() - c.ref).abs()
    assert bool((err <= c.bound).all()), float((err / c.bound).max())
    # the bound is a bound, not a tolerance: far below the 2e-2 / 6e-3 of the max-norm it replaces
    assert float(c.bound.max() / c.ref.abs().max()) < 5e-3


@pytest.mark.parametrize('run', WG_RAND, ids=repr)
def test_random_weight_gradient_case_reference_passes_its_own_bound(run):
    c = B.wg_case(run)
    assert c.share <= 1e-3, c.share
    n, cin, cout, k, stride, h, w = c.geom
    g32 = B.conv_wgrad(c.xo.q.float(), c.go.q.float(), (cout, cin, k, k), stride, k // 2)
    err = (g32.double() - c.ref).abs()
    assert bool((err <= c.bound).all()), float((err / c.bound).max())
    gb = c.go.v.float().sum(dim=(0, 2, 3)).double()
    assert bool(((gb - c.gb_ref).abs() <= c.gb_bound).all())
    assert float(c.bound.max() / c.ref.abs().max()) < 5e-3


@pytest.mark.parametrize('run', B.stat_runs(), ids=repr)
def test_statistics_bounds_are_fine_enough(run):
    """1e-4 of the channel's standard deviation (mean) / 1e-4 relative (variance) for the arithmetic alone: a coarser derivation would
    say nothing the fp32 family's 1e-5 tests do not"""
    c = B.run_case(run)
    sb = B.stats_bounds(c.ref, None, *B.run_stat_chain(run))
    assert float((sb.e_mean / sb.sigma).max()) <= 1e-4 and float((sb.e_var / sb.var).max()) <= 1e-4
    assert float(sb.sigma.min()) > 0


def test_trunk_walks_follow_the_share_rule():
    for sh, (rows, rounds) in B.TRUNK_WALK.items():
        tiles = sh[0] * (sh[1] // 8) * (sh[2] // 16)
        assert B.equal_shares(tiles, sh[3] if len(sh) == 4 else 256) == (rows, rounds), sh
    assert sorted(v[1] for v in B.TRUNK_WALK.values()) == [1, 1, 2, 2, 3]


def test_operand_builders_agree_with_the_oracle():
    n, c, h, w = 2, 8, 5, 7
    x, dy = B.rand((n, c, h, w), 1, 2.0), B.rand((n, c, h, w), 2)
    gamma, beta = B.rand((c,), 3) + 1.5, B.rand((c,), 4)
    slope = 0.2
    s32 = torch.tensor(slope)
    assert torch.equal(B.operand(B.ACT, x, slope=slope).v.float(), ops.leaky_relu(x, s32))
    assert torch.equal(B.operand(B.ACT, x, slope=slope).v.float(), ops.prelu(x, s32))
    t = B.rand((n, 16, h, w), 5)
    assert torch.equal(B.pixel_shuffle2(t), ops.pixel_shuffle(t, 2))
    wt = B.rand((4, c, 3, 3), 6)
    assert torch.equal(B.conv_fwd(x, wt, None, 1, 1), ops.conv2d(x, wt, None, 1, 1))
    # BatchNorm apply + activation = AFFINE_ACT with scale = gamma * invstd, shift = beta - mean * scale
    xd = x.double().requires_grad_(True)
    gd, bd = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    z, _, _ = ops.batch_norm(xd, gd, bd, torch.zeros(c).double(), torch.ones(c).double(), True)
    a = ops.leaky_relu(z, slope)
    mean, var = B.channel_stats(x)
    assert torch.allclose(mean, xd.detach().mean(dim=(0, 2, 3)), rtol=0, atol=1e-15)
    assert torch.allclose(var, ((xd.detach() - mean[None, :, None, None]) ** 2).mean(dim=(0, 2, 3)), rtol=1e-14, atol=0)
    invstd = torch.rsqrt(var + 1e-5)
    scale, shift = gamma.double() * invstd, beta.double() - mean * gamma.double() * invstd
    op = B.operand(B.AFFINE_ACT, x, pa=scale.float(), pd=shift.float(), slope=slope)
    assert float((op.v - a.detach()).abs().max()) < 1e-5
    # its backward = BNACT_BWD with the constants include/sisr_hip.h states, from the reductions of bnb_terms
    (a * dy.double()).sum().backward()
    k4 = torch.stack([scale, shift, mean, invstd])
    t = B.bnb_terms(dy, x, k4, float(s32))
    cnt = n * h * w
    sum_g, sum_gx = t.gg.sum(dim=(0, 2, 3)), t.ggx.sum(dim=(0, 2, 3))
    assert torch.allclose(sum_g, bd.grad, rtol=1e-6, atol=1e-9) and torch.allclose(sum_gx, gd.grad, rtol=1e-6, atol=1e-9)
    qa = gamma.double() * invstd
    qb = -gamma.double() * invstd ** 2 * sum_gx / cnt
    qd = -qa * sum_g / cnt - qb * mean
    f = lambda v: v.float()
    bw = B.operand(B.BNACT_BWD, dy, x, pa=f(qa), pb=f(qb), pd=f(qd), ps=f(scale), pt=f(shift), slope=slope)
    assert float((bw.v - xd.grad).abs().max()) < 1e-5
    # without the activation: BNBWD
    xd2 = x.double().requires_grad_(True)
    z2, _, _ = ops.batch_norm(xd2, gamma.double(), beta.double(), torch.zeros(c).double(), torch.ones(c).double(), True)
    (z2 * dy.double()).sum().backward()
    t2 = B.bnb_terms(dy, x, k4, None)
    qb2 = -gamma.double() * invstd ** 2 * t2.ggx.sum(dim=(0, 2, 3)) / cnt
    qd2 = -qa * t2.gg.sum(dim=(0, 2, 3)) / cnt - qb2 * mean
    bw2 = B.operand(B.BNBWD, dy, x, pa=f(qa), pb=f(qb2), pd=f(qd2))
    assert float((bw2.v - xd2.grad).abs().max()) < 1e-5
    # ACT_BWD / TANH_BWD against autograd of the oracle's activation and of tanh
    xr = x.double().requires_grad_(True)
    (ops.leaky_relu(xr, slope) * dy.double()).sum().backward()
    assert float((B.operand(B.ACT_BWD, dy, x, slope=slope).v - xr.grad).abs().max()) < 1e-6
    xr = x.double().requires_grad_(True)
    y = torch.tanh(xr)
    (y * dy.double()).sum().backward()
    assert float((B.operand(B.TANH_BWD, dy, y.detach().float()).v - xr.grad).abs().max()) < 1e-6
