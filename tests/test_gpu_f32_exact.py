"""GPU: exact-operand value tests of the fp32-tensor kernel family -- conv_fwd.hip, conv_wgrad.hip, conv_toimage.hip (f32 mode),
wgrad_toimage.hip (f32) and the persistent conv_trunk_f32.hip / wgrad_trunk_f32.hip in both precisions ('fp32': the fp32 matrix
instruction; 'bf16x3': the bf16 matrix instruction over hi / lo pairs) -- through the engine, against the float64 references of
tests/f32_cases.py (tests/test_f32_cases_cpu.py checks the cases' own conditions without a device).

Tier A, grid operands: every partial sum is exact and a bf16-representable operand splits as (x, 0), so BOTH precisions must equal
the float64 reference bit for bit, the bias gradient too, whatever the tile walk.  Tier S, two-piece operands ('bf16x3'): hi + lo
== v with lo != 0 on half the values; the result must equal the float64 hi hi + hi lo + lo hi bit for bit -- a lo read from the
wrong channel, tap or pixel, or a dropped cross term, differs by whole grid steps.  Tier B, ordinary random fp32 operands: the
derived element-wise bound.  Statistics and BatchNorm-backward rows are held to the bounds of their own arithmetic, the pixel count
and the number of rows exactly.  Every test first asserts the route its launch took; a second launch must give the same bits.

The generic kernels are kept on their route with SISR_TRUNK=0 and SISR_THIN=0; trunk shapes (n, h, w[, cap]) set
SISR_PERSIST_MAX_WG = cap (the fp32 kernel pairs workgroups: cap / 2 pixel-tile streams); the last conv's separate weight-gradient
kernel runs with SISR_TOIMAGE_BWD=0.  tanh epilogue: TANH_ULPS and its reasoning are those of tests/test_gpu_bf16_exact.py."""
import contextlib
import ctypes as C

import pytest
import torch

import bf16_cases as B
import f32_cases as F
import test_gpu_bf16_exact as T
from gpu_helpers import FakeConv, assert_within, nchw, pkg

pytestmark = pytest.mark.gpu
F32 = torch.float32
_operand, _dev, _merged, _mismatch, _unpack = T._operand, T._dev, T._merged, T._mismatch, T._unpack


@pytest.fixture(scope='module')
def E():
    return pkg('engine')


@pytest.fixture(scope='module')
def L():
    return pkg('_lib')


@pytest.fixture(autouse=True)
def _stop_at_a_gpu_error():
    """a launch that faulted poisons the process: end the run there instead of starting further launches"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit('GPU error: %s' % e, returncode=3)


@contextlib.contextmanager
def _build(E, run, monkeypatch):
    """the precision of the run and the knobs that send its launch to run.family"""
    if run.family == 'generic':
        for k in ('SISR_TRUNK', 'SISR_THIN'):
            monkeypatch.setenv(k, '0')
    if run.family == 'toimage':
        monkeypatch.setenv('SISR_TOIMAGE_BWD', '0')
    if run.family in ('trunk', 'toimage') and len(run.shape) == 4:
        monkeypatch.setenv('SISR_PERSIST_MAX_WG', str(run.shape[3]))
    E.set_precision(run.precision)
    try:
        yield
    finally:
        E.set_precision('fp32')


def _probe(E, d, p, role, op, out, bias=None, res=None, y_mode=None, epi=0, stats=False):
    """a copy of planned descriptor d filled the way engine.conv_forward / conv_dgrad fill it: for the route and *_eligible entry points"""
    d = E._copy_struct(d)
    op.fill(d)
    d.wpk = d.y = out.data_ptr()
    d.bias = None if bias is None else bias.data_ptr()
    d.res = None if res is None else res.data_ptr()
    if y_mode is not None:
        d.y_mode = y_mode
    d.epi_act = epi
    d.mfma_split = E.mfma_split()
    if role is not None:
        d.plan.variant = int(p.lanes[role]) | (2 * p.ldsimg[role])
    if stats:
        d.stat_part = d.cnt_part = out.data_ptr()
    return d


def _check_out(run, case, got_nchw, what):
    """tiers A and S: bit equality with the float64 reference; tier B: the derived bound of the run's precision"""
    assert got_nchw.dtype == F32
    if run.tier in ('grid', 'split'):
        assert torch.equal(got_nchw.double(), case.ref), (what, _mismatch(got_nchw.double(), case.ref, case.step))
    else:
        assert_within(got_nchw.double(), case.ref, case.bound[run.precision], '%r %s' % (run, what))


def _layer(E, case, run, **kw):
    n, cin, cout, k, stride, h, w = case.geom
    gm = E.ConvGeom(cin, cout, k, stride, k // 2, shuffle2=run.shuffle2)
    ref = FakeConv(case.w.cuda(), None if case.b is None else case.b.cuda(), gm)
    p = E.prepare_weights([(ref, n, h, w)], training=True, **kw)[0][0]
    assert all(kind == E.Kind.F32 for kind in p.kinds)
    if run.family == 'trunk' and not run.shuffle2:
        # the 64 -> 64 layers read the LDS-order weight image packed in the build's mode: 1 fp32 values, 2 split pairs
        assert p.ldsimg == ((2, 2) if run.precision == 'bf16x3' else (1, 1))
    return ref, p


FWD = [r for r in F.CONV_RUNS if r.role == 'fwd']
DGRAD = [r for r in F.CONV_RUNS if r.role == 'dgrad']


@pytest.mark.parametrize('run', FWD, ids=repr)
def test_forward(E, L, run, monkeypatch):
    """forward role: the prologues (and the skip sum formed in the staging, materialised bit for bit), bias, statistics, the
    PixelShuffle store, the NCHW image in and out with and without tanh"""
    with _build(E, run, monkeypatch):
        case = F.run_case(run)
        n, cin, cout, k, stride, h, w = case.geom
        ref, p = _layer(E, case, run)
        lib = L.lib()
        x_out = None
        if run.tag == 'image_in':
            op = _operand(E, L, run.pro, case.k, (n, h, w, cin), None, mode=L.X_NCHW)
        else:
            if run.pro == B.RES_AFFINE:
                x_out = torch.full((n, h, w, cin), float('nan'), dtype=F32, device='cuda')
            op = _operand(E, L, run.pro, case.k, (n, h, w, cin), F32, x_out=x_out)
        tanh = run.tag == 'tanh'
        kw = dict(bias=ref.bias)
        stats = F.stat_run(run)
        if F.image_out_run(run):
            kw.update(y_mode=L.Y_NCHW, epi=L.EPI_TANH if tanh else L.EPI_NONE)
        y, sp, cp = E.conv_forward(p, op, stats=stats, **kw)
        # ---- the route
        probe = _probe(E, p.plans[0], p, 0, op, y, bias=ref.bias, y_mode=kw.get('y_mode'), epi=kw.get('epi', 0), stats=stats)
        assert T.ROUTE_FAMILY[lib.sisr_conv2d_f32_route(C.byref(probe))] == run.family
        assert lib.sisr_conv2d_trunk_f32_eligible(C.byref(probe)) == int(run.family == 'trunk')                  # (1: its forward role)
        rows = F.TRUNK_WALK[run.shape][0] if run.family == 'trunk' and not run.shuffle2 else p.plans[0].plan.n_tiles
        # ---- values
        if F.image_out_run(run):
            assert tuple(y.shape) == case.oshape
            got = y.cpu()
        else:
            got = nchw(y).cpu()
        if tanh:
            want = torch.tanh(case.ref)
            err = (got.double() - want).abs()
            ulp = torch.exp2(torch.floor(torch.log2(want.abs().clamp_min(2.0 ** -126))) - 23)
            slack = torch.zeros_like(want) if run.tier == 'grid' else case.bound[run.precision]      # (tanh is 1-Lipschitz)
            print('%r tanhf: largest error %.2f fp32 ulps' % (run, float(((err - slack).clamp_min(0) / ulp).max())))
            assert bool((err <= slack + T.TANH_ULPS * ulp).all())
        else:
            _check_out(run, case, got, 'forward')
        if stats:
            assert sp.shape[0] == rows, 'statistics rows: %d, expected %d for this route' % (sp.shape[0], rows)
            tot, mean, var = _merged(sp, cp)
            assert tot == n * case.ref.shape[2] * case.ref.shape[3]
            sb = F.stats_bounds(case.ref, case.e_acc[run.precision] if run.tier == 'rand' else None, *F.run_stat_chain(run))
            assert_within(mean, sb.mean, sb.e_mean, '%r mean' % run)
            assert_within(var, sb.var, sb.e_var, '%r variance' % run)
        if x_out is not None:
            xo = nchw(x_out).cpu().double()
            if run.tier == 'rand':
                assert bool(sum(xo == c for c in [case.op.v] + case.op.evals).bool().all()), 'materialised skip sum: none of the fp32 evaluations'
            else:
                assert torch.equal(xo, case.a), 'materialised skip sum'
        y2, sp2, cp2 = E.conv_forward(p, op, stats=stats, **kw)
        assert torch.equal(y2, y) and (not stats or (torch.equal(sp2, sp) and torch.equal(cp2, cp))), 'two launches differ'


@pytest.mark.parametrize('run', DGRAD, ids=repr)
def test_data_gradient(E, L, run, monkeypatch):
    """data-gradient role: one- and two-tensor gradient prologues, the residual, the fused BatchNorm-backward reductions of the
    persistent kernel, stride 2 (four parity launches of the generic kernel), the un-shuffling view (four phase launches of the
    persistent kernel, each adding onto the one before)"""
    with _build(E, run, monkeypatch):
        case = F.run_case(run)
        n, cin, cout, k, stride, h, w = case.geom
        ref, p = _layer(E, case, run)
        lib = L.lib()
        ho, wo = (h + 2 * (k // 2) - k) // stride + 1, (w + 2 * (k // 2) - k) // stride + 1
        op = _operand(E, L, run.pro, case.k, (n, ho, wo, cout), F32, mode=L.X_UNSHUFFLE2 if run.shuffle2 else None)
        res = _dev(case.res, F32)
        res0 = None if res is None else res.clone()
        bnb = None
        if run.bnb:
            assert run.family == 'trunk' and E.can_fuse_bn_backward(p), 'this layer fuses the reductions'
            bs = case.bnb.slope
            bnb = (_dev(case.bnb.x, F32), case.bnb.k4.cuda(), None if bs is None else torch.tensor([bs], device='cuda'))
        elif run.family == 'generic':
            assert not E.can_fuse_bn_backward(p)                       # (conv_fwd.hip has no such epilogue)
        launch = lambda: E.conv_dgrad(p, op, res=res, bnb=bnb)
        r = launch()
        dx, part = r if bnb is not None else (r, None)
        # ---- the route
        if stride == 2:
            classes = p.plans[1]
            assert len(classes) == 4 and all(c is not None and c.kind == E.Kind.F32 for c in classes)
            for c in classes:
                probe = _probe(E, c.desc, p, None, op, dx, res=res)
                assert T.ROUTE_FAMILY[lib.sisr_conv2d_f32_route(C.byref(probe))] == 'generic'
        else:
            probe = _probe(E, p.plans[1], p, 1, op, dx, res=res)
            if bnb is not None:
                probe.bnb_x = probe.bnb_part = dx.data_ptr()
            assert T.ROUTE_FAMILY[lib.sisr_conv2d_f32_route(C.byref(probe))] == run.family
            assert lib.sisr_conv2d_trunk_f32_eligible(C.byref(probe)) == (2 if run.family == 'trunk' else 0)
        assert tuple(dx.shape) == (n, h, w, cin)
        _check_out(run, case, nchw(dx).cpu(), 'data gradient')
        assert res is None or torch.equal(res, res0), 'the residual was written'
        if bnb is not None:
            streams, tiles = F.TRUNK_WALK[run.shape]
            assert part is not None and part.shape[0] == 2 * streams, (None if part is None else part.shape, streams)
            s = part.double().cpu().sum(0)
            refs, bounds = F.bnb_reference(case, run.precision, *F.trunk_bnb_depth(tiles))
            for name, got, want, bound in zip(('sum g', 'sum g xhat', 'slope sum'), (s[:cin], s[cin:2 * cin], s[2 * cin:]), refs, bounds):
                assert_within(got, want, bound, '%r %s' % (run, name))
        r2 = launch()
        dx2, part2 = r2 if bnb is not None else (r2, None)
        assert torch.equal(dx2, dx) and (part is None or torch.equal(part2, part)), 'two launches differ'


# ---- weight gradients ---------------------------------------------------------------------------------------------------------------
def _wg_setup(E, L, run):
    """-> (case, ref, p, x_op, g_op, route family) under the precision and knobs already set"""
    case = F.wg_case(run)
    n, cin, cout, k, stride, h, w = case.geom
    ho, wo = (h + 2 * (k // 2) - k) // stride + 1, (w + 2 * (k // 2) - k) // stride + 1
    wt, b = B.make_weights(cout, cin, k, 'grid', 8000 + run.seed)
    ref = FakeConv(wt.cuda(), b.cuda(), E.ConvGeom(cin, cout, k, stride, k // 2, shuffle2=run.tag == 'up'))
    p = E.prepare_weights([(ref, n, h, w)], training=True, need_dgrad=False)[0][0]
    assert p.kinds[2] == E.Kind.F32
    if run.tag == 'image_in':
        x_op = _operand(E, L, run.xpro, case.kx, (n, h, w, cin), None, mode=L.X_NCHW)
    else:
        x_op = _operand(E, L, run.xpro, case.kx, (n, h, w, cin), F32)
    if run.family == 'toimage' or run.tag == 'padded':
        g_op = _operand(E, L, run.gpro, case.kg, (n, ho, wo, cout), None, mode=L.X_NCHW)
    else:
        g_op = _operand(E, L, run.gpro, case.kg, (n, ho, wo, cout), F32, mode=L.X_UNSHUFFLE2 if run.tag == 'up' else None)
    g = E._copy_struct(p.plans[2])
    x_op.fill(g)
    g_op.fill(g, g=True)
    g.mfma_split = E.mfma_split()
    lib = L.lib()
    route = T.ROUTE_FAMILY[lib.sisr_wgrad_f32_route(C.byref(g))]
    assert lib.sisr_wgrad_trunk_f32_eligible(C.byref(g)) == int(run.family == 'trunk')
    return case, ref, p, x_op, g_op, route


def _check_wg(run, case, gw, gb):
    if run.tier in ('grid', 'split'):
        assert torch.equal(gw.double(), case.ref), ('weight gradient', _mismatch(gw.double(), case.ref, case.step))
        assert torch.equal(gb.double(), case.gb_ref), 'bias gradient'
    else:
        assert_within(gw.double(), case.ref, case.bound[run.precision], '%r weight gradient' % run)
        assert_within(gb.double(), case.gb_ref, case.gb_bound, '%r bias gradient' % run)


@pytest.mark.parametrize('run', F.WG_RUNS, ids=repr)
def test_weight_gradient(E, L, run, monkeypatch):
    """weight and bias gradient: both operands lazy, the slabs summed in a fixed order; the bias gradient is the sum of the fp32 values"""
    with _build(E, run, monkeypatch):
        case, ref, p, x_op, g_op, route = _wg_setup(E, L, run)
        assert route == run.family, 'the launch ran on the %s kernel' % route
        red = E.conv_wgrad(p, x_op, g_op)
        gw, gb = _unpack(E, p, ref, red)
        _check_wg(run, case, gw, gb)
        gw2, gb2 = _unpack(E, p, ref, E.conv_wgrad(p, x_op, g_op))
        assert torch.equal(gw2, gw) and torch.equal(gb2, gb), 'two launches differ'


@pytest.mark.parametrize('tier,precision', list(F.TRUNK_BATCH), ids=lambda v: v)
def test_trunk_weight_gradients_of_three_layers_in_one_launch(E, L, tier, precision, monkeypatch):
    """sisr_wgrad_trunk_f32_batch: every member bit-equal to its single launch and to the reference"""
    runs = F.TRUNK_BATCH[(tier, precision)]
    with _build(E, runs[0], monkeypatch):
        members = []
        for r in runs:
            case, ref, p, x_op, g_op, route = _wg_setup(E, L, r)
            assert route == 'trunk'
            members.append((r, case, ref, p, x_op, g_op))
        wb, pending = E.WgradDeepBatch(), E.PendingSlabs()
        before = E.KERNEL_COUNTS.get('wgrad_trunk_batch', 0)
        reds = [wb.add(p, x_op, g_op) for _, _, _, p, x_op, g_op in members]
        assert all(r is not None for r in reds) and len(wb.trunk) == 3 and wb.items == []
        wb.run(pending)
        assert E.KERNEL_COUNTS.get('wgrad_trunk_batch', 0) == before + 1 and len(pending.jobs) == 3
        pending.flush()
        for (r, case, ref, p, x_op, g_op), red in zip(members, reds):
            gw, gb = _unpack(E, p, ref, red)
            _check_wg(r, case, gw, gb)
            gw1, gb1 = _unpack(E, p, ref, E.conv_wgrad(p, x_op, g_op))
            assert torch.equal(gw, gw1) and torch.equal(gb, gb1), 'a member differs from its single launch'
