"""CPU: the conditions on the seeded cases of tests/test_gpu_fc_head.py (tests/fc_head_cases.py) that keep that file from hiding a
failure.  Tier A: inside the 2^22 budget, every operand and reference representable in fp32, torch's own fp32 evaluation bit-equal to
the float64 reference -- and each defect the grids are there to catch (a lost K step, a shifted weight row, swapped batch rows, a
dropped odd row, a dropped wave partition, the wrong LeakyReLU' at zero) moves the reference by at least one grid step.  Tier B:
torch's fp32 evaluation, in its own order, inside every bound.  Shapes: each forward shape has the slicing property it was chosen for,
computed with the kernel's own formula."""
import pytest
import torch

import fc_head_cases as C

F32 = torch.float32
ids = lambda s: 'x'.join(map(str, s))                   # noqa: E731


def _moved(a, b):
    return float((a - b).abs().max())


# ---- budget and representability -------------------------------------------------------------------------------------------------
def _exact(*tensors):
    for t in tensors:
        assert C.representable(t.double()), 'not representable in fp32'


@pytest.mark.parametrize('shape', C.FORWARD, ids=ids)
def test_forward_grid_case_is_exact(shape):
    c = C.forward_case(shape, 'grid')
    b = C.budget('forward', c)
    print('forward %s: budget %.3g' % (shape, b))
    assert b < C.BUDGET
    for with_b1 in (False, True):
        r = C.forward_ref(c, with_b1=with_b1)
        _exact(c.x, c.w1, c.b1, c.w2, c.b2, r.h1)
        h32 = c.x @ c.w1.t() + (c.b1 if with_b1 else 0.0)
        assert h32.dtype == F32 and torch.equal(h32.double(), r.h1)
    assert bool((c.b1 != 0).any()) and float(c.b2) != 0                # a null bias and a given one differ


@pytest.mark.parametrize('shape', C.BACKWARD, ids=ids)
def test_backward_grid_case_is_exact(shape):
    c = C.backward_case(shape, 'grid')
    b = C.budget('backward', c)
    print('backward %s: budget %.3g' % (shape, b))
    assert b < C.BUDGET
    r = C.backward_ref(c)
    _exact(c.g, c.y, c.h1, c.w2, r.d2, r.d1, r.dW2, r.db2, r.db1)
    # both zeros, negative and positive values are there, and no gradient row is switched off
    z = c.h1 == 0
    assert bool((z & ~torch.signbit(c.h1)).any()) and bool((z & torch.signbit(c.h1)).any())
    assert bool((c.h1 < 0).any()) and bool((c.h1 > 0).any()) and bool((r.d2 != 0).all())
    # torch in fp32, its own order and its own leaky_relu
    h = c.h1.clone().requires_grad_(True)
    w = c.w2.clone().requires_grad_(True)
    t = torch.nn.functional.leaky_relu(h, c.slope) @ w
    t.backward(r.d2.float())
    assert torch.equal(h.grad.double(), r.d1) and torch.equal(w.grad.double(), r.dW2)


@pytest.mark.parametrize('shape', C.DGRAD, ids=ids)
def test_dgrad_grid_case_is_exact(shape):
    c = C.dgrad_case(shape, 'grid')
    b = C.budget('dgrad', c)
    print('dgrad %s: budget %.3g' % (shape, b))
    assert b < C.BUDGET
    r = C.dgrad_ref(c)
    _exact(c.d1, c.w1, r.dx)
    assert torch.equal((c.d1 @ c.w1).double(), r.dx)


@pytest.mark.parametrize('shape', C.ROWS, ids=ids)
def test_rows_grid_case_is_exact(shape):
    c = C.rows_case(shape, 'grid')
    b = C.budget('rows', c)
    print('rows %s: budget %.3g' % (shape, b))
    assert b < C.BUDGET
    for scale in C.SCALES:
        r = C.rows_ref(c, scale)
        _exact(c.dy, c.x, r.dW)
        assert torch.equal(((c.dy.t() @ c.x) * scale).double(), r.dW)


@pytest.mark.parametrize('shape', C.TWO_PATHS, ids=ids)
def test_two_path_grid_case_is_exact(shape):
    c = C.two_path_case(shape, 'grid')
    assert C.budget('two_path', c) < C.BUDGET
    f = c.fwd
    _exact(c.d1, C.forward_ref(f).h1, C.dgrad_ref(f, d1=c.d1, w1=f.w1).dx, C.wgrad_ref(c.d1, f.x)[0])


# ---- mutations: each named defect moves the float64 reference by at least one grid step -------------------------------------------
@pytest.mark.parametrize('shape', C.FORWARD + C.TWO_PATHS, ids=ids)
def test_forward_mutations_move_the_reference(shape):
    B, K, N = shape
    c = C.forward_case(shape, 'grid')
    ref = C.forward_ref(c).h1
    # the final K step of one slice dropped: every non-empty slice in turn
    lens, ends = C.slices(K), C.slice_ends(K)
    for sl in range(C.NSL):
        if lens[sl]:
            x = c.x.clone()
            x[:, 16 * (ends[sl] - 1):16 * ends[sl]] = 0
            assert _moved(C.forward_ref(c, x=x).h1, ref) >= c.step, ('last step of slice', sl)
    # weight row n read as n + 1
    assert _moved(C.forward_ref(c, w1=torch.roll(c.w1, -1, 0)).h1, ref) >= c.step
    # two batch rows swapped
    if B > 1:
        x = c.x.clone()
        x[[0, 1]] = c.x[[1, 0]]
        assert _moved(C.forward_ref(c, x=x).h1, ref) >= c.step


@pytest.mark.parametrize('shape', C.DGRAD + C.TWO_PATHS, ids=ids)
def test_dgrad_mutations_move_the_reference(shape):
    B, K, N = shape
    c = C.dgrad_case(shape, 'grid')
    ref = C.dgrad_ref(c).dx
    for wave in range(4):                                              # one of the four wave partitions of N dropped
        d1 = c.d1.clone()
        d1[:, wave * (N // 4):(wave + 1) * (N // 4)] = 0
        assert _moved(C.dgrad_ref(c, d1=d1).dx, ref) >= c.step, wave
    assert _moved(C.dgrad_ref(c, w1=torch.roll(c.w1, -1, 0)).dx, ref) >= c.step
    if B > 1:
        d1 = c.d1.clone()
        d1[[0, 1]] = c.d1[[1, 0]]
        assert _moved(C.dgrad_ref(c, d1=d1).dx, ref) >= c.step


@pytest.mark.parametrize('shape', [s for s in C.ROWS if s[0] % 2], ids=ids)
def test_rows_mutation_the_odd_last_row_dropped(shape):
    c = C.rows_case(shape, 'grid')
    for scale in C.SCALES:
        assert _moved(C.rows_ref(c, scale, rows=shape[0] - 1).dW, C.rows_ref(c, scale).dW) >= c.step * scale


@pytest.mark.parametrize('shape', C.BACKWARD, ids=ids)
def test_backward_mutation_slope_one_at_zero(shape):
    c = C.backward_case(shape, 'grid')
    ref, mut = C.backward_ref(c), C.backward_ref(c, zero_gate=1.0)
    assert _moved(mut.d1, ref.d1) >= c.step
    assert _moved(mut.db1, ref.db1) >= c.step


# ---- tier B: torch's fp32 evaluation lies inside every bound ----------------------------------------------------------------------
def _inside(got32, ref, bound, what):
    assert got32.dtype == F32
    err = (got32.double() - ref).abs()
    print('%s: torch fp32 uses %.3f of the bound' % (what, float((err / bound.clamp_min(1e-300)).max())))
    assert bool(torch.isfinite(bound).all()) and bool((bound > 0).any()) and bool((err <= bound).all()), what


@pytest.mark.parametrize('shape', C.FORWARD + C.TWO_PATHS, ids=ids)
def test_forward_random_case_reference_passes_its_own_bound(shape):
    c = C.forward_case(shape, 'rand')
    slope = torch.tensor(c.slope, dtype=F32)
    for with_b1 in (False, True):
        for with_b2 in (False, True):
            r = C.forward_ref(c, with_b1, with_b2)
            h = c.x @ c.w1.t() + (c.b1 if with_b1 else 0.0)
            y = torch.sigmoid(torch.where(h > 0, h, slope * h) @ c.w2 + (c.b2 if with_b2 else 0.0))
            _inside(h, r.h1, r.bound_h, 'h1 %s' % (shape,))
            _inside(y, r.y, r.bound_y, 'y %s' % (shape,))
    # the grid tier's y has a bound too (h1 exact, the second layer rounds)
    g = C.forward_case(shape, 'grid')
    r = C.forward_ref(g)
    h = g.x @ g.w1.t() + g.b1
    _inside(torch.sigmoid(torch.where(h > 0, h, 0.25 * h) @ g.w2 + g.b2), r.y, r.bound_y, 'grid y %s' % (shape,))
    assert float(r.y.min()) > 0.02 and float(r.y.max()) < 0.98, 'a saturated sigmoid hides its sum'


@pytest.mark.parametrize('shape', C.BACKWARD, ids=ids)
def test_backward_random_case_reference_passes_its_own_bound(shape):
    c = C.backward_case(shape, 'rand')
    r = C.backward_ref(c)
    slope = torch.tensor(c.slope, dtype=F32)
    d2 = c.g * c.y * (1 - c.y)
    d1 = d2[:, None] * c.w2[None, :] * torch.where(c.h1 > 0, torch.ones((), dtype=F32), slope)
    _inside(d1, r.d1, r.bound_d1, 'd1 %s' % (shape,))
    _inside(d2 @ torch.where(c.h1 > 0, c.h1, slope * c.h1), r.dW2, r.bound_dW2, 'dW2 %s' % (shape,))
    _inside(d2.sum().reshape(1), r.db2, r.bound_db2, 'db2 %s' % (shape,))
    _inside(d1.sum(0), r.db1, r.bound_db1, 'db1 %s' % (shape,))
    assert bool((c.h1 == 0).any())


@pytest.mark.parametrize('shape', C.DGRAD + C.TWO_PATHS, ids=ids)
def test_dgrad_random_case_reference_passes_its_own_bound(shape):
    c = C.dgrad_case(shape, 'rand')
    r = C.dgrad_ref(c)
    _inside(c.d1 @ c.w1, r.dx, r.bound, 'dx %s' % (shape,))


@pytest.mark.parametrize('shape', C.ROWS, ids=ids)
def test_rows_random_case_reference_passes_its_own_bound(shape):
    c = C.rows_case(shape, 'rand')
    for scale in C.SCALES:
        r = C.rows_ref(c, scale)
        _inside((c.dy.t() @ c.x) * scale, r.dW, r.bound, 'dW %s scale %g' % (shape, scale))


def test_random_operands_are_on_no_coarse_grid():
    c = C.forward_case(C.FORWARD[2], 'rand')
    for t in (c.x, c.w1, c.b1, c.w2):
        assert not torch.equal(t.to(torch.bfloat16).float(), t)


# ---- the property each forward shape is chosen for --------------------------------------------------------------------------------
def _paths(K):
    """per wave slice: (trips of the unrolled loop, steps of the tail loop)"""
    return [(n // C.FH_UNROLL, n % C.FH_UNROLL) for n in C.slices(K)]


def test_forward_shapes_reach_every_loop_combination():
    want = {16: dict(lens={0, 1}, empty=15, unrolled=False, tail=True),          # tail loop only, 15 empty slices
            64: dict(lens={0, 1}, empty=12, unrolled=False, tail=True),          # tail only, 12 empty
            2048: dict(lens={8}, empty=0, unrolled=True, tail=False),            # unrolled only
            2816: dict(lens={11}, empty=0, unrolled=True, tail=True),            # 8 + 3 in every slice
            2880: dict(lens={11, 12}, empty=0, unrolled=True, tail=True),        # uneven slices
            4160: dict(lens={16, 17}, empty=0, unrolled=True, tail=True)}        # slices with and without a tail side by side
    assert sorted(want) == sorted(s[1] for s in C.FORWARD)
    for K, w in want.items():
        lens, paths = C.slices(K), _paths(K)
        assert sum(lens) == K // 16 and C.slice_ends(K)[-1] == K // 16
        assert set(lens) == w['lens'] and lens.count(0) == w['empty'], (K, lens)
        assert any(t for t, _ in paths) == w['unrolled'] and any(r for _, r in paths) == w['tail'], (K, paths)
        assert max(lens) == -(-(K // 16) // C.NSL)                       # what depth_h1 counts
    # a slice that is tail only beside none that is unrolled; a slice that is both; slices of both kinds in one launch
    assert all(t == 0 for t, _ in _paths(16) + _paths(64))
    assert all(t == 1 and r == 3 for t, r in _paths(2816))
    assert {p for p in _paths(4160)} == {(2, 0), (2, 1)}
    for K in (192, 2880):                                                # the two-path shapes: 12 steps, four empty slices; as above
        assert K in [s[1] for s in C.TWO_PATHS]
    assert C.slices(192).count(0) == 4 and set(C.slices(192)) == {0, 1}


def test_other_shapes_reach_their_edges():
    # backward and finish kernels stride N by 256: a partial workgroup alone, a partial last one, full ones
    assert sorted({(n + 255) // 256 for _, n in C.BACKWARD}) == [1, 2] and {n % 256 for _, n in C.BACKWARD} == {16, 128, 0}
    assert {b for b, _ in C.BACKWARD} >= {1, 16} and {s[0] for s in C.FORWARD} >= {1, 16} and {s[0] for s in C.DGRAD} >= {1, 16}
    assert {s[2] % 256 for s in C.FORWARD} >= {16, 128, 144, 0}
    # data gradient: trips of 32 rows per wave
    assert [s[2] // 4 // 32 for s in C.DGRAD] == [1, 1, 3, 9] and all(s[1] % 64 == 0 and s[2] % 128 == 0 for s in C.DGRAD)
    # rows kernel: below, at and past the 64-row round, odd and even, the cap
    rows = [s[0] for s in C.ROWS]
    assert rows == [1, 2, 63, 64, 65, 129, 255, 256] and max(rows) == C.FR_MAXROWS
    assert all(s[1] % 128 == 0 and s[2] % 64 == 0 for s in C.ROWS)
    assert all(b <= C.FH_B for b, _, _ in C.FORWARD + C.DGRAD + C.TWO_PATHS) and all(b <= C.FH_B for b, _ in C.BACKWARD)
