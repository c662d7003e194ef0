"""CPU: the conditions on the seeded cases of tests/test_gpu_f32_exact.py (tests/f32_cases.py) that keep that file from hiding a
failure.  Tier A: inside the 2^22 budget, operands exact after the prologue in every evaluation order, the fp32 and the emulated
three-product CPU contractions bit-equal to the float64 reference.  Tier S: the prologue gives back the two-piece target in every
evaluation order, hi + lo == v with lo != 0 on at least a quarter of the kept values, every output element sees a cross term, the
budget over the three product grids is below 2^22, and the emulated fp32 contraction equals the float64 reference -- which the
dropped lo lo term separates from the full product by whole grid steps.  Tier B: operands not bf16-representable, the fp32 / emulated
CPU evaluation inside the case's bound, and the bound far below the max-norm tolerance it stands beside (the ratio is printed)."""
import pytest
import torch

import bf16_cases as B
import f32_cases as C
import test_gpu_trunk_f32_walk as W

CONV = {t: [r for r in C.CONV_RUNS if r.tier == t] for t in ('grid', 'split', 'rand')}
WG = {t: [r for r in C.all_wg_runs() if r.tier == t] for t in ('grid', 'split', 'rand')}


def _unique(runs):
    """one run per case: the two precisions of a grid case share it"""
    seen, out = set(), []
    for r in runs:
        if r.seed not in seen:
            seen.add(r.seed)
            out.append(r)
    return out


def _every_evaluation_gives(op, target):
    """the one-rounding value and both fp32 evaluations of the prologue (fused, stepwise) are the target, bit for bit"""
    return torch.equal(op.v, target) and all(torch.equal(e, target) for e in op.evals)


def _against_the_max_norm(run, what, bound, ref):
    """The largest bound of the case over the error the max-norm tolerance beside it allows, printed.  It is NOT asserted to be small,
    because it is not: gamma_K is the worst case of ANY summation order, K u = 3.4e-5 for the 576 terms of a trunk element before the
    factor S / max|ref| (3 to 5 here), while the 1e-5 / 4e-5 / 1e-4 of the trunk tests are empirical (errors of random signs grow
    like sqrt(K) u).  Measured over the committed cases: 9 to 15 on the trunk convs (68 to 90 on the upscale conv's data gradient,
    2304 terms), 1 to 30 on the weight gradients, 0.6 to 1.5 beside the generic kernels' 2e-4.  What tier B adds to the max-norm
    tests is therefore the element's own scale (an element far smaller than the tensor's largest is held to ITS sum of magnitudes),
    not a smaller figure; the sharp checks are tiers A and S.  Asserted: the bound is finite and positive wherever terms are."""
    key = (run.family, what, run.precision) if run.family == 'trunk' else (run.family, what)
    ratio = float(bound.max() / ref.abs().max()) / C.MAXNORM_TOL[key]
    print('%r: largest bound / max-norm tolerance %.3f' % (run, ratio))
    assert bool(torch.isfinite(bound).all()) and bool((bound > 0).all())


@pytest.mark.parametrize('run', CONV['grid'], ids=repr)
def test_grid_conv_case_is_exact(run):
    c = C.run_case(run)
    assert c.budget < C.BUDGET, c.budget
    for t in (c.a, c.w.double()) + (() if c.res is None else (c.res.double(),)):
        assert torch.equal(B.bf(t), t), 'an operand is not representable in bf16'
    assert _every_evaluation_gives(c.op, c.a)
    y = C.emulated(c, run.precision)
    assert y.dtype == torch.float32 and torch.equal(y.double(), c.ref)
    lo = C.split(c.a)[1]
    assert not bool(lo.any())


@pytest.mark.parametrize('run', CONV['split'], ids=repr)
def test_two_piece_conv_case_is_exact(run):
    c = C.run_case(run)
    assert c.budget < C.BUDGET, c.budget
    print('%r: budget %.3g, product step 2^%d, lo share %.2f / %.2f' % (run, c.budget, round(torch.log2(torch.tensor(c.step)).item()), *c.lo_share))
    assert _every_evaluation_gives(c.op, c.target)
    for (hi, lo), t in zip(c.hi_lo, (c.a, c.w.double())):
        assert torch.equal(hi + lo, t), 'hi + lo != v'
    assert min(c.lo_share) >= 0.25, c.lo_share
    assert float((c.cross > 0).double().mean()) >= 0.995               # (a corner pixel sees four taps of nine: now and then no kept pair)
    y = C.emulated(c, 'bf16x3')
    assert y.dtype == torch.float32 and torch.equal(y.double(), c.ref)
    assert c.dropped >= c.step                                          # the full product differs: the reference is the kernel's three terms


@pytest.mark.parametrize('run', CONV['rand'], ids=repr)
def test_random_conv_case_reference_passes_its_own_bound(run):
    c = C.run_case(run)
    assert not torch.equal(B.bf(c.a), c.a) and not torch.equal(B.bf(c.w), c.w)
    y = C.emulated(c, run.precision)
    err, bound = (y.double() - c.ref).abs(), c.bound[run.precision]
    assert bool((err <= bound).all()), float((err / bound).max())
    _against_the_max_norm(run, 'conv', bound, c.ref)


@pytest.mark.parametrize('run', _unique(WG['grid']), ids=repr)
def test_grid_weight_gradient_case_is_exact(run):
    c = C.wg_case(run)
    assert c.budget < C.BUDGET, c.budget
    for o in (c.xo, c.go):
        assert torch.equal(B.bf(o.v), o.v) and _every_evaluation_gives(o, o.v)
    for pr in C.PRECISIONS:
        g = C.emulated_wgrad(c, pr)
        assert g.dtype == torch.float32 and torch.equal(g.double(), c.ref)
    assert torch.equal(c.go.v.float().sum(dim=(0, 2, 3)).double(), c.gb_ref)


@pytest.mark.parametrize('run', WG['split'], ids=repr)
def test_two_piece_weight_gradient_case_is_exact(run):
    c = C.wg_case(run)
    assert c.budget < C.BUDGET, c.budget
    print('%r: budget %.3g, lo share %.2f / %.2f' % (run, c.budget, *c.lo_share))
    for o, t in zip((c.xo, c.go), c.targets):
        assert _every_evaluation_gives(o, t)
    for (hi, lo), o in zip(c.hi_lo, (c.xo, c.go)):
        assert torch.equal(hi + lo, o.v), 'hi + lo != v'
    assert min(c.lo_share) >= 0.25, c.lo_share
    assert float((c.cross > 0).double().mean()) > 0.99                   # (a tap at the image edge may see no kept pixel pair)
    g = C.emulated_wgrad(c, 'bf16x3')
    assert g.dtype == torch.float32 and torch.equal(g.double(), c.ref)
    assert torch.equal(c.go.v.float().sum(dim=(0, 2, 3)).double(), c.gb_ref)
    assert c.dropped >= c.step


@pytest.mark.parametrize('run', WG['rand'], ids=repr)
def test_random_weight_gradient_case_reference_passes_its_own_bound(run):
    c = C.wg_case(run)
    assert not torch.equal(B.bf(c.xo.v), c.xo.v) and not torch.equal(B.bf(c.go.v), c.go.v)
    g = C.emulated_wgrad(c, run.precision)
    err, bound = (g.double() - c.ref).abs(), c.bound[run.precision]
    assert bool((err <= bound).all()), float((err / bound).max())
    gb = c.go.v.float().sum(dim=(0, 2, 3)).double()
    assert bool(((gb - c.gb_ref).abs() <= c.gb_bound).all())
    _against_the_max_norm(run, 'wgrad', bound, c.ref)


@pytest.mark.parametrize('run', [r for r in _unique(C.CONV_RUNS) if C.stat_run(r) and r.tier != 'rand'], ids=repr)
def test_statistics_bounds_are_fine_enough(run):
    """1e-4 of the channel's standard deviation (mean) / 1e-4 relative (variance) for the arithmetic alone on conv_fwd.hip, as the bf16
    file; 3e-4 on conv_trunk_f32.hip, whose lane keeps ONE chain over all its tiles (96 values on the walk of six)"""
    c = C.run_case(run)
    sb = C.stats_bounds(c.ref, None, *C.run_stat_chain(run))
    assert float(sb.sigma.min()) > 0
    fine = 3e-4 if run.family == 'trunk' else 1e-4
    assert float((sb.e_mean / sb.sigma).max()) <= fine and float((sb.e_var / sb.var).max()) <= fine


def test_trunk_walks_follow_the_share_rule():
    assert C.WALK_SHAPES == W.WALK_SHAPES and C.UP_SHAPES == W.UP_SHAPES
    for sh, (streams, rounds) in C.TRUNK_WALK.items():
        tiles = sh[0] * (sh[1] // 8) * (sh[2] // 16)
        assert B.equal_shares(tiles, (sh[3] if len(sh) == 4 else 256) // 2) == (streams, rounds), sh
        assert W.WALKS[sh] == streams
    assert sorted(v[1] for v in C.TRUNK_WALK.values()) == [1, 1, 2, 3, 6]


def test_every_listed_geometry_is_there():
    """the tables hold what they are meant to hold"""
    import test_gpu_kernels as K
    assert all(g in K.CONV_CASES for g in C.RAGGED_CHANNELS)
    fams = {(r.family, r.role, r.tier, r.precision) for r in C.CONV_RUNS + C.all_wg_runs()}
    for role in ('fwd', 'dgrad', 'wgrad'):
        assert {('trunk', role, 'grid', 'fp32'), ('trunk', role, 'grid', 'bf16x3'), ('trunk', role, 'split', 'bf16x3'), ('trunk', role, 'rand', 'fp32'),
                ('trunk', role, 'rand', 'bf16x3'), ('generic', role, 'grid', 'fp32'), ('generic', role, 'rand', 'fp32')} <= fams
    assert all(max(r.shape[:3]) <= 48 or r.family != 'trunk' for r in C.CONV_RUNS + C.all_wg_runs())
    # tier S reaches both weight paths: the packed split image (64 -> 64) and the in-kernel split (the upscale conv)
    s = [r for r in C.CONV_RUNS if r.tier == 'split']
    assert any(r.shuffle2 for r in s) and any(not r.shuffle2 for r in s)
