"""GPU: value tests of the discriminator's classifier head (csrc/fc_head.hip) -- sisr_fc_head_forward, sisr_fc_head_backward,
sisr_fc1_dgrad and sisr_fc_wgrad_rows, one entry point at a time through the C ABI, against float64 on the CPU.  The inputs,
references and bounds are tests/fc_head_cases.py; tests/test_fc_head_cases_cpu.py checks their own conditions without a device and
tests/test_fc_head_args_cpu.py the refusals (no test here passes a misaligned pointer, B > 16 or more than 256 rows).

What every case does (tests/gpu_helpers.py):
  * every output lives in a Buf between two sentinel guards and every call goes through run2: status 0, guards intact, two launches
    from the same pre-fill bit-identical (the file header of fc_head.hip promises a fixed order).  The Bufs hold exactly B x N, B x K,
    N, 1 elements, so a written row >= B lands in a guard;
  * tier 'grid': torch.equal with the float64 reference, no tolerance (all products exact fp32, all partial sums inside the budget);
  * tier 'rand': element by element inside 2 gamma_D sum|terms| with D counted from the kernel (fc_head_cases.depth_*);
    assert_within prints the worst error / bound ratio.  y passes through a sigmoid and has a bound in both tiers.
The shapes are the smallest at which each path can go wrong (fc_head_cases.FORWARD ... ROWS say which path each one is for)."""
import itertools
from types import SimpleNamespace as NS

import pytest
import torch

import fc_head_cases as C
from gpu_helpers import SENT, Buf, assert_within, pkg, run2
from test_gpu_glue import _fc_rows_per_split

pytestmark = pytest.mark.gpu

ids = lambda s: 'x'.join(map(str, s))                   # noqa: E731


@pytest.fixture(scope='module')
def lib():
    return pkg('_lib').lib()


@pytest.fixture(scope='module')
def E():
    return pkg('engine')


def _st():
    return torch.cuda.current_stream().cuda_stream


def dev(t):
    return t.to(torch.float32).contiguous().cuda()


def _check(got, ref, bound, what):
    """tier A (bound None): bit equality with the float64 reference; tier B: element by element inside the bound"""
    got = got.detach().cpu().reshape(ref.shape)
    if bound is None:
        assert torch.equal(got.double(), ref), '%s: %d of %d elements differ, worst by %.3e' % (
            what, int((got.double() != ref).sum()), ref.numel(), float((got.double() - ref).abs().max()))
    else:
        assert_within(got, ref, bound, what)


def _untouched(buf):
    return bool((buf.body == SENT).all())


# ---- forward -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tier', C.TIERS)
@pytest.mark.parametrize('shape', C.FORWARD, ids=ids)
def test_forward(lib, shape, tier):
    B, K, N = shape
    c = C.forward_case(shape, tier)
    xd, w1d, b1d, w2d, b2d = (dev(t) for t in (c.x, c.w1, c.b1, c.w2, c.b2))
    assert lib.sisr_fc_head_ws_floats(N) == C.FH_KQ * C.FH_B * N
    h1, y, ws = Buf(B * N), Buf(B), Buf(C.FH_KQ * C.FH_B * N)

    def call(with_b1, w2, with_b2):
        return lib.sisr_fc_head_forward(xd.data_ptr(), w1d.data_ptr(), b1d.data_ptr() if with_b1 else None, w2,
                                        b2d.data_ptr() if with_b2 else None, c.slope, h1.ptr(), y.ptr(), ws.ptr(), B, K, N, _st())

    for with_b1, with_b2 in itertools.product((1, 0), (1, 0)):
        r = C.forward_ref(c, with_b1, with_b2)
        what = 'forward %s %s b1=%d b2=%d' % (shape, tier, with_b1, with_b2)
        run2(lambda: call(with_b1, w2d.data_ptr(), with_b2), [h1, y, ws])
        _check(h1.body, r.h1, r.bound_h, what + ' h1')
        assert_within(y.cpu(), r.y, r.bound_y, what + ' y')
        # the sharper form of the same check: the finish kernel feeds the h1 it stores to the second layer, so y is held to the
        # float64 second layer of THAT h1, without the worst-case error of h1 carried through sum |W2|
        y_own, bound_own = C.second_layer(h1.cpu().view(B, N).double(), None, c.w2.double(), c.b2.double() if with_b2 else None,
                                          C.f32(c.slope))
        assert_within(y.cpu(), y_own, bound_own, what + ' y from the stored h1')
        # the partial sums: every slot written, the batch rows >= B hold the zeros the kernel multiplied
        part = ws.body.view(C.FH_KQ, C.FH_B, N)
        assert not bool((part == SENT).any()) and bool((part[:, B:] == 0).all())
        if tier == 'grid':                                  # ... and each K quarter is exact on its own (four slices each)
            ends = [0] + [16 * e for e in C.slice_ends(K)[3::4]]
            want = torch.stack([c.x.double()[:, a:b] @ c.w1.double()[:, a:b].t() for a, b in zip(ends, ends[1:])])
            assert torch.equal(part[:, :B].cpu().double(), want), what + ' K quarters'
    # the first layer alone: W2 null, y keeps its sentinel
    for with_b1 in (1, 0):
        r = C.forward_ref(c, with_b1, True)
        run2(lambda: call(with_b1, None, 1), [h1, y, ws])
        _check(h1.body, r.h1, r.bound_h, 'forward %s %s b1=%d first layer only, h1' % (shape, tier, with_b1))
        assert _untouched(y), 'y written although W2 is null'


# ---- backward behind h1 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tier', C.TIERS)
@pytest.mark.parametrize('shape', C.BACKWARD, ids=ids)
def test_backward(lib, shape, tier):
    B, N = shape
    c = C.backward_case(shape, tier)
    r = C.backward_ref(c)
    gd, yd, hd, w2d = (dev(t) for t in (c.g, c.y, c.h1, c.w2))
    assert torch.equal(torch.signbit(hd.cpu()), torch.signbit(c.h1))                  # the zeros kept their signs on the way
    d1, dW2, db2, db1 = Buf(B * N), Buf(N), Buf(1), Buf(N)
    for null in ('', 'db2', 'db1'):
        run2(lambda: lib.sisr_fc_head_backward(gd.data_ptr(), yd.data_ptr(), hd.data_ptr(), w2d.data_ptr(), c.slope, d1.ptr(), dW2.ptr(),
                                               None if null == 'db2' else db2.ptr(), None if null == 'db1' else db1.ptr(), B, N, _st()),
             [d1, dW2, db2, db1])
        what = 'backward %s %s null=%s' % (shape, tier, null or 'none')
        bound = (lambda k: None) if tier == 'grid' else (lambda k: getattr(r, 'bound_' + k))
        _check(d1.body, r.d1, bound('d1'), what + ' d1')
        _check(dW2.body, r.dW2, bound('dW2'), what + ' dW2')
        for name, buf in (('db2', db2), ('db1', db1)):
            if null == name:
                assert _untouched(buf), name + ' written although null was passed'
            else:
                _check(buf.body, getattr(r, name), bound(name), what + ' ' + name)


# ---- data gradient of the first layer ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tier', C.TIERS)
@pytest.mark.parametrize('shape', C.DGRAD, ids=ids)
def test_fc1_dgrad(lib, shape, tier):
    B, K, N = shape
    c = C.dgrad_case(shape, tier)
    r = C.dgrad_ref(c)
    d1d, w1d = dev(c.d1), dev(c.w1)
    dx = Buf(B * K)
    run2(lambda: lib.sisr_fc1_dgrad(d1d.data_ptr(), w1d.data_ptr(), dx.ptr(), B, K, N, _st()), [dx])
    _check(dx.body, r.dx, r.bound, 'fc1_dgrad %s %s' % (shape, tier))


# ---- weight gradient from many rows --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tier', C.TIERS)
@pytest.mark.parametrize('shape', C.ROWS, ids=ids)
def test_fc_wgrad_rows(lib, shape, tier):
    rows, K, N = shape
    c = C.rows_case(shape, tier)
    dyd, xd = dev(c.dy), dev(c.x)
    dW = Buf(N * K)
    for scale in C.SCALES:
        r = C.rows_ref(c, scale)
        run2(lambda: lib.sisr_fc_wgrad_rows(dyd.data_ptr(), xd.data_ptr(), scale, dW.ptr(), rows, K, N, _st()), [dW])
        _check(dW.body, r.dW, r.bound, 'fc_wgrad_rows %s %s scale=%g' % (shape, tier, scale))


# ---- two independent implementations, one reference ----------------------------------------------------------------------------------
def _generic_depths(lib, K, N):
    """chain lengths of the generic kernels (csrc/layout_fc.hip), as tests/test_gpu_glue.py counts them: forward 4 ceil(K / 1024) + 10;
    data gradient rows + splits; weight gradient 16; bias gradient B"""
    rows, _ = _fc_rows_per_split(K, N)
    return NS(fwd=lambda k: 4 * ((k + 1023) // 1024) + 10, dgrad=rows + lib.sisr_fc_dgrad_splits(K, N), wgrad=16)


@pytest.mark.parametrize('shape', C.TWO_PATHS, ids=ids)
def test_head_and_generic_paths_are_exact_on_grid_operands(lib, E, shape):
    """tier A: h1, dx = d1 W1 and dW1 = d1^T x of the head path (fc_head.hip + the generic weight gradient) and of the generic path
    the discriminator falls back to both equal the float64 reference bit for bit"""
    B, K, N = shape
    assert E.fc_head_ok(B, K, N)
    c = C.two_path_case(shape, 'grid')
    f = c.fwd
    x, w1, b1, w2, b2, d1 = (dev(t) for t in (f.x, f.w1, f.b1, f.w2.view(1, N), f.b2, c.d1))
    h1_ref = C.forward_ref(f).h1
    dx_ref = C.dgrad_ref(f, d1=c.d1, w1=f.w1).dx
    dw_ref = C.wgrad_ref(c.d1, f.x)[0]
    h1_head, _ = E.fc_head_forward(x, w1, b1, w2, b2, f.slope)
    h1_gen = E.fc_forward(x, w1, b1)
    dx_gen, dw_gen, db_gen = E.fc_backward(d1, x, w1)
    for what, got, ref in (('head h1', h1_head, h1_ref), ('generic h1', h1_gen, h1_ref), ('head dx', E.fc1_dgrad(d1, w1), dx_ref),
                           ('generic dx', dx_gen, dx_ref), ('head dW1', E.fc_wgrad_only(d1, x, w1), dw_ref),
                           ('generic dW1', dw_gen, dw_ref), ('generic db1', db_gen, c.d1.double().sum(0))):
        _check(got, ref, None, '%s %s' % (what, shape))


@pytest.mark.parametrize('shape', C.TWO_PATHS, ids=ids)
def test_head_and_generic_paths_stay_inside_their_own_bounds(lib, E, shape):
    """tier B: the whole forward + backward of both paths as discriminator_engine wires them.  Each stage is held to the float64
    evaluation of ITS OWN inputs (the fp32 tensors the path handed it), inside the bound of the kernel that ran it."""
    B, K, N = shape
    c = C.two_path_case(shape, 'rand')
    f = c.fwd
    slope = C.f32(f.slope)
    x, w1, b1, w2, b2, g = (dev(t) for t in (f.x, f.w1, f.b1, f.w2.view(1, N), f.b2, c.g.view(B, 1)))
    fr = C.forward_ref(f)
    w2_64, b2_64 = f.w2.double(), f.b2.double()
    cpu = lambda t: t.detach().cpu()                      # noqa: E731
    tag = lambda path, k: '%s %s %s' % (path, k, shape)   # noqa: E731

    def stage_case(h1, y):
        return NS(g=c.g, y=cpu(y).reshape(B), h1=cpu(h1), w2=f.w2, slope=f.slope, tier='rand')

    # the head path
    h1, y = E.fc_head_forward(x, w1, b1, w2, b2, f.slope)
    d1, dw2, db2, db1 = E.fc_head_backward(g, y, h1, w2, f.slope)
    dx, dw1 = E.fc1_dgrad(d1, w1), E.fc_wgrad_only(d1, x, w1)
    assert_within(cpu(h1), fr.h1, fr.bound_h, tag('head', 'h1'))
    y_ref, y_bound = C.second_layer(cpu(h1).double(), None, w2_64, b2_64, slope)
    assert_within(cpu(y).reshape(B), y_ref, y_bound, tag('head', 'y'))
    r = C.backward_ref(stage_case(h1, y))
    for k, got in (('d1', d1), ('dW2', dw2), ('db2', db2), ('db1', db1)):
        assert_within(cpu(got).reshape(getattr(r, k).shape), getattr(r, k), getattr(r, 'bound_' + k), tag('head', k))
    rd = C.dgrad_ref(NS(tier='rand'), d1=cpu(d1), w1=f.w1)
    assert_within(cpu(dx), rd.dx, rd.bound, tag('head', 'dx'))
    dw_ref, dw_s = C.wgrad_ref(cpu(d1), f.x)
    assert_within(cpu(dw1), dw_ref, C.bnd(16, dw_s), tag('head', 'dW1'))

    # the generic path
    D = _generic_depths(lib, K, N)
    D2 = _generic_depths(lib, N, 1)
    h1g = E.fc_forward(x, w1, b1)
    yg = E.fc_forward(h1g, w2, b2, in_slope=f.slope, sigmoid=True)
    d2g = E.act_bwd(g, yg, 1)
    dx2g, dw2g, db2g = E.fc_backward(d2g, h1g, w2, in_slope=f.slope)
    d1g = E.act_bwd(dx2g, h1g, 0, f.slope)
    dxg, dw1g, db1g = E.fc_backward(d1g, x, w1)
    assert_within(cpu(h1g), fr.h1, C.bnd(D.fwd(K), fr.s_h), tag('generic', 'h1'))
    y_ref, y_bound = C.second_layer(cpu(h1g).double(), None, w2_64, b2_64, slope, depth=D.fwd(N) + 1)       # + 1: slope * h on load
    assert_within(cpu(yg).reshape(B), y_ref, y_bound, tag('generic', 'y'))
    r = C.backward_ref(stage_case(h1g, yg))
    assert_within(cpu(d2g).reshape(B), r.d2, C.bnd(C.D_D2, r.d2.abs()), tag('generic', 'd2'))
    # from here on the stages read the path's own d2 (here it is a tensor in memory, in the head's backward kernel a register)
    d2 = cpu(d2g).reshape(B).double()
    a = C.lrelu(cpu(h1g).double(), slope)
    assert_within(cpu(dw2g).reshape(N), d2 @ a, C.bnd(D.wgrad + 1, d2.abs() @ a.abs()), tag('generic', 'dW2'))
    assert_within(cpu(db2g).reshape(1), d2.sum().reshape(1), C.bnd(B, d2.abs().sum().reshape(1)), tag('generic', 'db2'))
    gate = torch.where(cpu(h1g).double() > 0, torch.ones((), dtype=torch.float64), torch.full((), slope, dtype=torch.float64))
    d1_ref = d2[:, None] * w2_64[None, :] * gate
    assert_within(cpu(d1g), d1_ref, C.bnd(D2.dgrad + 1, d1_ref.abs()), tag('generic', 'd1'))
    d1_64 = cpu(d1g).double()
    assert_within(cpu(dxg), d1_64 @ f.w1.double(), C.bnd(D.dgrad, d1_64.abs() @ f.w1.double().abs()), tag('generic', 'dx'))
    dw_ref, dw_s = C.wgrad_ref(cpu(d1g), f.x)
    assert_within(cpu(dw1g), dw_ref, C.bnd(D.wgrad, dw_s), tag('generic', 'dW1'))
    assert_within(cpu(db1g), d1_64.sum(0), C.bnd(B, d1_64.abs().sum(0)), tag('generic', 'db1'))
    # the LeakyReLU gates of the two paths can differ only where h1 itself is within the two bounds of zero
    differ = (cpu(h1) > 0) != (cpu(h1g) > 0)
    assert bool((fr.h1.abs()[differ] <= fr.bound_h[differ] + C.bnd(D.fwd(K), fr.s_h)[differ]).all())
