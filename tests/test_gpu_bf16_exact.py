"""GPU: exact-operand value tests of the bf16 matrix-core kernel family (conv_bf16 / conv_trunk / conv_deep / conv_thin / conv_toimage
and wgrad_bf16 / wgrad_trunk / wgrad_deep / wgrad_thin / wgrad_toimage .hip) through the engine, against the float64 references of
tests/bf16_cases.py (tests/test_bf16_cases_cpu.py checks the cases' own conditions without a device).

Tier A, grid operands: every partial sum is exact in fp32, so fp32 results must EQUAL the float64 reference, bf16-stored results its
round-to-nearest-even, the bias gradient bit for bit, whatever the tile walk; statistics and BatchNorm-backward rows are held to the
bounds of their own arithmetic and the count exactly.  Tier B, ordinary random operands (not bf16-representable where the tensor is
fp32): the derived bound gamma_K S + A element by element -- this tier keeps the rounding of the staging itself under test.
Every test first asserts the route its launch took; a second launch must give the same bits.

Trunk shapes: conv_trunk.hip shares its tiles by sisr_equal_shares(tiles, slots) -- rounds = ceil(tiles / slots), workgroups =
ceil(tiles / rounds) -- where the fp32 kernel pairs workgroups.  (1, 16, 16) therefore runs with a cap of 1, not 2 (two tiles on ONE
workgroup: the walk of two), (1, 24, 16, 2) is the uneven walk 2 + 1, (3, 24, 48, 10) gives 9 workgroups x 3 tiles strided across
rows and images.

tanh epilogue: with it off the grid cases are bit-equal (the sharp check).  With it on the error is the library's tanhf, not project
code; the ROCm installation carries no copy of the HIP math accuracy tables, so TANH_ULPS is twice the largest error measured on an
MI355X over these cases."""
import ctypes as C

import pytest
import torch

import bf16_cases as B
from gpu_helpers import FakeConv, assert_within, nchw, nhwc, pkg

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
TANH_ULPS = 2.5        # measured on an MI355X over the to-image and generic cases below: at most 1.21 fp32 ulps of the result; doubled
ROUTE_FAMILY = ['generic', 'deep', 'toimage', 'trunk', 'thin']      # run.family by _lib.ROUTE_* (enum SisrRoute)


@pytest.fixture(scope='module')
def E():
    e = pkg('engine')
    e.set_precision('bf16')
    yield e
    e.set_precision('fp32')


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


def _env(monkeypatch, family, storage, shape):
    """the knobs that send a launch to `family`"""
    monkeypatch.setenv('SISR_STORAGE', storage)
    if family == 'generic':
        for k in ('SISR_TRUNK', 'SISR_DEEP', 'SISR_WGRAD_DEEP', 'SISR_THIN'):
            monkeypatch.setenv(k, '0')
    if family in ('trunk', 'thin', 'toimage') and len(shape) == 4:
        monkeypatch.setenv('SISR_PERSIST_MAX_WG', str(shape[3]))


def _dev(t, dt=None, layout='nhwc'):
    if t is None:
        return None
    t = nhwc(t) if layout == 'nhwc' and t.dim() == 4 else t
    return t.cuda().to(dt) if dt is not None else t.cuda()


def _operand(E, L, pro, k, dims, dt, mode=None, x_out=None):
    """the engine's lazy operand of a case's inputs k (tests/bf16_cases.operand's arguments), tensors NHWC in `dt` -- or, mode =
    L.X_NCHW, the fp32 NCHW image as it is"""
    layout = 'nchw' if mode == L.X_NCHW else 'nhwc'
    x1, x2 = _dev(k['x1'], dt, layout), _dev(k.get('x2'), dt, layout)
    c = {n: _dev(k.get(n)) for n in ('pa', 'pb', 'pd', 'ps', 'pt')}
    slope = k.get('slope')
    slope = None if slope is None else torch.tensor([slope], device='cuda')
    if pro == B.RES_AFFINE:
        return E.Operand.res_affine(x1, slope, x2, c['pa'], c['pd'], x_out)
    return E.Operand(x1, dims, pro=pro, mode=L.X_NHWC if mode is None else mode, x2=x2, slope=slope, **c)


def _merged(sp, cp):
    cnt, mean_t, m2_t = cp.double().cpu(), sp[:, 0].double().cpu(), sp[:, 1].double().cpu()
    tot = cnt.sum()
    mean = (cnt[:, None] * mean_t).sum(0) / tot
    return float(tot), mean, (m2_t + cnt[:, None] * (mean_t - mean) ** 2).sum(0) / tot


def _probe(E, p, role, op, out, res=None, y_mode=None, epi=0, stats=False):
    """a copy of the planned descriptor filled the way engine.conv_forward / conv_dgrad fill it: for the *_eligible entry points"""
    d = E._copy_struct(p.plans[role])
    op.fill(d)
    d.wpk = d.y = out.data_ptr()
    d.y_bf16, d.res_bf16 = int(out.dtype == BF16), int(res is not None and res.dtype == BF16)
    d.res = None if res is None else res.data_ptr()
    if y_mode is not None:
        d.y_mode = y_mode
    d.epi_act = epi
    d.plan.variant = int(p.lanes[role])
    if stats:
        d.stat_part = d.cnt_part = out.data_ptr()
    return d


def _check_out(run, case, got_nchw, what):
    """tier A: bit equality with the float64 reference (its round-to-nearest-even for a bf16 tensor); tier B: the derived bound"""
    if run.tier == 'grid':
        if got_nchw.dtype == BF16:
            assert torch.equal(got_nchw, case.ref.to(BF16)), (what, _mismatch(got_nchw.double(), case.stored, case.step))
        else:
            assert torch.equal(got_nchw.double(), case.ref), (what, _mismatch(got_nchw.double(), case.ref, case.step))
    else:
        assert_within(got_nchw.double(), case.ref, case.bound, '%r %s' % (run, what))


def _mismatch(got, ref, step):
    """which elements differ, and by how many grid steps: the pattern names the tile edge, tap or wave"""
    bad = (got != ref).nonzero()
    d = ((got - ref) / step)[got != ref]
    return 'differ: %d of %d, first at %s, by %s grid steps (largest %.1f)' % (len(bad), got.numel(), bad[:4].tolist(), d[:4].tolist(),
                                                                              float(d.abs().max()))


def _check_stats(run, case, sp, cp, rows):
    assert sp.shape[0] == rows, 'statistics rows: %d, expected %d for this route' % (sp.shape[0], rows)
    tot, mean, var = _merged(sp, cp)
    assert tot == case.ref.shape[0] * case.ref.shape[2] * case.ref.shape[3]
    sb = B.stats_bounds(case.ref, None if run.tier == 'grid' else case.e_acc, *B.run_stat_chain(run))
    assert_within(mean, sb.mean, sb.e_mean, '%r mean' % run)
    assert_within(var, sb.var, sb.e_var, '%r variance' % run)


def _check_bnb(run, case, part, rows, family, tiles_per_row=1, cout_tile=128):
    assert part is not None and (rows is None or part.shape[0] == rows), (None if part is None else part.shape, rows)
    cch = case.ref.shape[1]
    s = part.double().cpu().sum(0)
    refs, bounds = B.bnb_reference(case, *B.bnb_depth(family, cout_tile, tiles_per_row))
    for name, got, ref, bound in zip(('sum g', 'sum g xhat', 'slope sum'), (s[:cch], s[cch:2 * cch], s[2 * cch:]), refs, bounds):
        assert_within(got, ref, bound, '%r %s' % (run, name))


FWD = [r for r in B.CONV_RUNS if r.role == 'fwd']
DGRAD = [r for r in B.CONV_RUNS if r.role == 'dgrad']


def _layer(E, case, run, n, h, w):
    geom = case.geom
    gm = E.ConvGeom(geom[1], geom[2], geom[3], geom[4], geom[3] // 2, shuffle2=run.shuffle2)
    ref = FakeConv(case.w.cuda(), None if case.b is None else case.b.cuda(), gm)
    return ref, E.prepare_weights([(ref, n, h, w)], training=True)[0][0]


@pytest.mark.parametrize('run', FWD, ids=repr)
def test_forward(E, L, run, monkeypatch):
    """forward role of every family: the three prologues (and the skip sum formed in the staging), bias, statistics, the
    PixelShuffle store, the NCHW fp32 image with and without tanh"""
    _env(monkeypatch, run.family, run.storage, run.shape)
    case = B.run_case(run)
    n, cin, cout, k, stride, h, w = case.geom
    dt = BF16 if run.storage == 'bf16' else F32
    ref, p = _layer(E, case, run, n, h, w)
    lib = L.lib()
    x_out = None
    if run.family == 'thin':
        op = _operand(E, L, run.pro, case.k, (n, h, w, 3), None, mode=L.X_NCHW)
    else:
        if run.pro == B.RES_AFFINE:
            x_out = torch.empty((n, h, w, cin), dtype=dt, device='cuda')
        op = _operand(E, L, run.pro, case.k, (n, h, w, cin), dt, x_out=x_out)
    tanh = run.tag == 'tanh'
    kw = dict(bias=ref.bias)
    stats = run in B.stat_runs()
    if B.image_out_run(run):
        kw.update(y_mode=L.Y_NCHW, epi=L.EPI_TANH if tanh else L.EPI_NONE)
    y, sp, cp = E.conv_forward(p, op, stats=stats, **kw)
    # ---- the route
    probe = _probe(E, p, 0, op, y, y_mode=kw.get('y_mode'), epi=kw.get('epi', 0), stats=stats)
    route = (lib.sisr_conv2d_bf16_route if p.kinds[0].bf16 else lib.sisr_conv2d_f32_route)(C.byref(probe))
    if run.family == 'deep':
        assert p.kinds[0] == E.Kind.DEEP
        rows = p.plans[0].deep.tiles_x * p.plans[0].deep.tiles_q
    else:
        assert p.kinds[0] == (E.Kind.F32 if run.family == 'thin' else E.Kind.BF16) and ROUTE_FAMILY[route] == run.family
        assert route != L.ROUTE_TRUNK or lib.sisr_conv2d_trunk_eligible(C.byref(probe)) == 1              # (1: its forward role)
        rows = p.plans[0].plan.n_tiles
        if run.family == 'trunk' and not run.shuffle2:
            rows = B.TRUNK_WALK[run.shape][0]
    # ---- values
    if B.image_out_run(run):
        assert y.dtype == F32 and tuple(y.shape) == case.oshape
        got = y.cpu()
    else:
        assert y.dtype == dt if run.family != 'thin' else y.dtype == BF16
        got = nchw(y).cpu()
    if tanh:
        want = torch.tanh(case.ref)
        err = (got.double() - want).abs()
        ulp = torch.exp2(torch.floor(torch.log2(want.abs().clamp_min(2.0 ** -126))) - 23)
        slack = torch.zeros_like(want) if run.tier == 'grid' else case.bound        # (tanh is 1-Lipschitz)
        print('%r tanhf: largest error %.2f fp32 ulps' % (run, float(((err - slack).clamp_min(0) / ulp).max())))
        assert bool((err <= slack + TANH_ULPS * ulp).all())
    else:
        _check_out(run, case, got, 'forward')
    if stats:
        _check_stats(run, case, sp, cp, rows)
    if x_out is not None:
        xo = nchw(x_out).cpu().double()
        if run.tier == 'grid':
            assert torch.equal(xo, case.op.q), 'materialised skip sum'
        else:
            assert bool(sum(xo == c for c in case.op.alts).bool().all()), 'materialised skip sum: none of the fp32 evaluations'
    y2, sp2, cp2 = E.conv_forward(p, op, stats=stats, **kw)
    assert torch.equal(y2, y) and (not stats or (torch.equal(sp2, sp) and torch.equal(cp2, cp))), 'two launches differ'


@pytest.mark.parametrize('run', DGRAD, ids=repr)
def test_data_gradient(E, L, run, monkeypatch):
    """data-gradient role: one- and two-tensor gradient prologues, the residual, the fused BatchNorm-backward reductions, stride 2
    (four parity classes: four launches on the generic kernel, one on conv_deep.hip), the un-shuffling view, tanh' over the image"""
    _env(monkeypatch, run.family, run.storage, run.shape)
    case = B.run_case(run)
    n, cin, cout, k, stride, h, w = case.geom
    dt = BF16 if run.storage == 'bf16' else F32
    ref, p = _layer(E, case, run, n, h, w)
    lib = L.lib()
    ho, wo = (h + 2 * (k // 2) - k) // stride + 1, (w + 2 * (k // 2) - k) // stride + 1
    if run.family == 'thin':
        op = _operand(E, L, run.pro, case.k, (n, h, w, 3), None, mode=L.X_NCHW)
    else:
        op = _operand(E, L, run.pro, case.k, (n, ho, wo, cout), dt, mode=L.X_UNSHUFFLE2 if run.shuffle2 else None)
    res = _dev(case.res, dt)
    bnb = None
    if run.bnb and E.can_fuse_bn_backward(p):
        bs = case.bnb.slope
        bnb = (_dev(case.bnb.x, dt), case.bnb.k4.cuda(), None if bs is None else torch.tensor([bs], device='cuda'))
    if run.bnb and (run.family != 'generic' or run.shape in (B.GENERIC[0], B.RAGGED)):
        assert bnb is not None, 'this layer fuses the reductions'
    launch = lambda: E.conv_dgrad(p, op, res=res, bnb=bnb)
    r = launch()
    dx, part = r if bnb is not None else (r, None)
    # ---- the route
    kind, rows, tpr, cout_tile = p.kinds[1], None, 1, 64
    if run.family == 'deep':
        # (the data gradient of a 32-channel input has 32 output channels: conv_deep.hip takes them in 64s, the generic kernel runs)
        assert kind == (E.Kind.BF16 if cin % 64 else E.Kind.DEEP if stride == 1 else E.Kind.DEEP_S2X4)
        d1 = p.plans[1]
        cout_tile = (d1.desc if kind == E.Kind.DEEP_S2X4 else d1).deep.BN if kind.deep else d1.plan.nsub * 32
    elif run.family == 'thin':
        assert kind == E.Kind.F32 and lib.sisr_conv2d_thin_eligible(C.byref(_probe(E, p, 1, op, dx))) == 1
    elif stride == 2:
        assert all(c is not None and c.kind == E.Kind.BF16 for c in p.plans[1])
    else:
        assert kind == E.Kind.BF16
        probe = _probe(E, p, 1, op, dx, res=res)
        if bnb is not None:
            probe.bnb_x = probe.bnb_part = dx.data_ptr()
            probe.bnbx_bf16 = int(dt == BF16)
        role = lib.sisr_conv2d_trunk_eligible(C.byref(probe))
        assert role == (2 if run.family == 'trunk' else 0)
        if run.family == 'trunk' and not run.shuffle2:
            rows, tpr = B.TRUNK_WALK[run.shape]
        elif run.family == 'generic':
            rows, cout_tile = p.plans[1].plan.n_tiles, p.plans[1].plan.nsub * 32
    assert dx.dtype == (BF16 if run.family == 'thin' else dt) and tuple(dx.shape) == (n, h, w, cin)
    _check_out(run, case, nchw(dx).cpu(), 'data gradient')
    if bnb is not None:
        _check_bnb(run, case, part, rows, 'trunk' if run.family == 'trunk' else 'generic', tpr, cout_tile)
    r2 = launch()
    dx2, part2 = r2 if bnb is not None else (r2, None)
    assert torch.equal(dx2, dx) and (part is None or torch.equal(part2, part)), 'two launches differ'


# ---- weight gradients ---------------------------------------------------------------------------------------------------------------
def _wg_setup(E, L, run, monkeypatch, slab_bf16='0'):
    """-> (case, ref, p, x_op, g_op, route) with the knobs of the run's family set; SISR_SLAB_BF16=0: fp32 slabs, exact on a grid"""
    _env(monkeypatch, run.family, run.storage, run.shape)
    monkeypatch.setenv('SISR_SLAB_BF16', slab_bf16)
    case = B.wg_case(run)
    n, cin, cout, k, stride, h, w = case.geom
    ho, wo = (h + 2 * (k // 2) - k) // stride + 1, (w + 2 * (k // 2) - k) // stride + 1
    dt = BF16 if run.storage == 'bf16' else F32
    wt, b = B.make_weights(cout, cin, k, 'grid', 8000 + run.seed)
    ref = FakeConv(wt.cuda(), b.cuda(), E.ConvGeom(cin, cout, k, stride, k // 2, shuffle2=run.tag == 'up'))
    p = E.prepare_weights([(ref, n, h, w)], training=True, need_dgrad=False)[0][0]
    if run.family == 'thin':
        x_op = _operand(E, L, run.xpro, case.kx, (n, h, w, 3), None, mode=L.X_NCHW)
    else:
        x_op = _operand(E, L, run.xpro, case.kx, (n, h, w, cin), dt)
    if run.family == 'toimage' or run.tag == 'padded':
        g_op = _operand(E, L, run.gpro, case.kg, (n, ho, wo, cout), None, mode=L.X_NCHW)
    else:
        # ('up': the upscale conv's gradient is the [n, 2 h, 2 w, 64] tensor behind the PixelShuffle, read through the un-shuffling view)
        g_op = _operand(E, L, run.gpro, case.kg, (n, ho, wo, cout), BF16 if run.family == 'thin' else dt,
                        mode=L.X_UNSHUFFLE2 if run.tag == 'up' else None)
    g = E._copy_struct(p.plans[2])
    x_op.fill(g)
    g_op.fill(g, g=True)
    bf16 = p.kinds[2].bf16
    route = ROUTE_FAMILY[(L.lib().sisr_wgrad_bf16_route if bf16 else L.lib().sisr_wgrad_f32_route)(C.byref(g))]
    # (of the fp32 dispatcher's kernels only the thin one belongs to this family)
    return case, ref, p, x_op, g_op, route if bf16 or route == 'thin' else 'f32'


def _unpack(E, p, ref, red):
    wg = E.WeightGradBatch()
    wg.add(p, red)
    gw, gb = wg.run()[id(ref)]
    return gw.cpu(), gb.cpu()


def _generic_bias_chain(g):
    """longest chain of additions of the bias gradient on wgrad_bf16.hip, from the launch's plan g (so this bound leans on the planner of
    the library under test, and is applied here only: tests/bf16_cases.py keeps the any-order bound over all pixels): a thread adds
    the values of its 4 channels over its share of every tile of its workgroup -- 256 / G pixels per step, G = 8 .. 32 channel groups:
    at most tile pixels / 8 per tile --, the workgroup sums its 256 / G <= 32 thread partials in sequence, the slab reduction adds
    n_slabs rows; + 5 for the roundings of the prologue itself (contracted or not)"""
    tile = g.TN * g.TH * ((g.TW + 15) // 16 * 16)
    return -(-tile // 8) * -(-g.n_tiles // g.grid_x) + 32 + g.n_slabs + 5


def _check_wg(run, case, gw, gb, plan=None):
    if run.tier != 'grid' and run.family == 'generic':
        chain = min(_generic_bias_chain(plan), case.terms + 5)
        assert_within(gb.double(), case.gb_ref, chain * B.U * case.go.mag.sum(dim=(0, 2, 3)), '%r bias gradient, chain of %d' % (run, chain))
    if run.tier == 'grid':
        assert torch.equal(gw.double(), case.ref), ('weight gradient', _mismatch(gw.double(), case.ref, case.step))
        assert torch.equal(gb.double(), case.gb_ref), 'bias gradient'
    else:
        assert_within(gw.double(), case.ref, case.bound, '%r weight gradient' % run)
        assert_within(gb.double(), case.gb_ref, case.gb_bound, '%r bias gradient' % run)


@pytest.mark.parametrize('run', B.WG_RUNS, ids=repr)
def test_weight_gradient(E, L, run, monkeypatch):
    """weight and bias gradient of every family with fp32 slabs: both operands lazy; the bias gradient is summed BEFORE the rounding"""
    case, ref, p, x_op, g_op, route = _wg_setup(E, L, run, monkeypatch)
    assert route == run.family, 'the launch ran on the %s kernel' % route
    before = E.KERNEL_COUNTS.get('wgrad_deep', 0)
    red = E.conv_wgrad(p, x_op, g_op)
    assert E.KERNEL_COUNTS.get('wgrad_deep', 0) == before + (run.family == 'deep')
    if run.tag == 'padded':
        assert p.plans[2].Cout == 4
    gw, gb = _unpack(E, p, ref, red)
    _check_wg(run, case, gw, gb, p.plans[2])
    assert torch.equal(E.conv_wgrad(p, x_op, g_op), red), 'two launches differ'


@pytest.mark.parametrize('run', B.SLAB_RUNS, ids=repr)
def test_bf16_slabs_round_each_partial_once(E, L, run, monkeypatch):
    """the default stores every workgroup's partial gradient P_s as bf16.  The fp32 slabs of the SISR_SLAB_BF16=0 launch are read from
    its pending reduction (their sum has just been proven exact); the default launch's result must be sum_s bf16(P_s) up to the fp32
    sum of n_slabs terms -- n_slabs u sum_s |P_s| -- and its bias row, which stays fp32, bit-equal"""
    case, ref, p, x_op, g_op, route = _wg_setup(E, L, run, monkeypatch, '0')
    assert route == run.family
    pend = E.PendingSlabs()
    red0 = E.conv_wgrad(p, x_op, g_op, defer=pend)
    (slab, red_t, n_slabs, stride, lead), = pend.jobs
    assert lead == 0 and red_t is red0
    torch.cuda.synchronize()
    parts = slab.double().cpu()
    pend.flush()
    assert pend.jobs == []
    elems = p.plans[2].slab_elems
    gw0, gb0 = _unpack(E, p, ref, red0)
    assert torch.equal(gw0.double(), case.ref) and torch.equal(gb0.double(), case.gb_ref)
    assert torch.equal(parts.sum(0), red0.double().cpu())
    # the default
    case, ref1, p1, x_op, g_op, route = _wg_setup(E, L, run, monkeypatch, '1')
    pend = E.PendingSlabs()
    red1 = E.conv_wgrad(p1, x_op, g_op, defer=pend)
    (slab1, _, n_slabs1, stride1, lead1), = pend.jobs
    assert (n_slabs1, stride1, lead1) == (n_slabs, stride, elems), 'the default launch must write the same slabs, their lead as bf16'
    pend.flush()
    want = B.bf(parts[:, :elems].float()).double().sum(0)
    bound = n_slabs * B.U * parts[:, :elems].abs().sum(0)
    assert_within(red1[:elems].double().cpu(), want, bound, '%r packed gradient from bf16 slabs' % run)
    assert torch.equal(red1[elems:], red0[elems:]), 'bias row'


def _batch_members(E, L, runs, monkeypatch):
    out = []
    for r in runs:
        case, ref, p, x_op, g_op, route = _wg_setup(E, L, r, monkeypatch)
        assert route == r.family
        out.append((r, case, ref, p, x_op, g_op))
    return out


def _check_batch(E, members, reds, pending):
    pending.flush()
    for (r, case, ref, p, x_op, g_op), red in zip(members, reds):
        gw, gb = _unpack(E, p, ref, red)
        _check_wg(r, case, gw, gb)
        gw1, gb1 = _unpack(E, p, ref, E.conv_wgrad(p, x_op, g_op))
        assert torch.equal(gw, gw1) and torch.equal(gb, gb1), 'a member differs from its single launch'


def test_trunk_weight_gradients_of_three_layers_in_one_launch(E, L, monkeypatch):
    monkeypatch.setenv('SISR_WGRAD_BATCH_TRUNK_PIXELS', '0')          # (small trunk layers would go to wgrad_deep's batch)
    members = _batch_members(E, L, B.TRUNK_BATCH, monkeypatch)
    wb, pending = E.WgradDeepBatch(), E.PendingSlabs()
    before = E.KERNEL_COUNTS.get('wgrad_trunk_batch', 0)
    reds = [wb.add(p, x_op, g_op) for _, _, _, p, x_op, g_op in members]
    assert all(r is not None for r in reds) and len(wb.trunk) == 3 and wb.items == []
    wb.run(pending)
    assert E.KERNEL_COUNTS.get('wgrad_trunk_batch', 0) == before + 1 and len(pending.jobs) == 3
    _check_batch(E, members, reds, pending)


@pytest.mark.parametrize('stride', [1, 2])
def test_deep_weight_gradients_of_three_layers_in_one_launch(E, L, stride, monkeypatch):
    members = _batch_members(E, L, B.DEEP_BATCH[stride], monkeypatch)
    wb, pending = E.WgradDeepBatch(), E.PendingSlabs()
    before = E.KERNEL_COUNTS.get('wgrad_deep_batch', 0)
    reds = [wb.add(p, x_op, g_op) for _, _, _, p, x_op, g_op in members]
    assert all(r is not None for r in reds) and len(wb.items) == 3
    wb.run(pending)
    assert E.KERNEL_COUNTS.get('wgrad_deep_batch', 0) == before + 1 and len(pending.jobs) == 3
    _check_batch(E, members, reds, pending)


def _wg_run(family, shape, xpro, gpro, tag=''):
    r, = [r for r in B.WG_RUNS if (r.family, r.shape, r.xpro, r.gpro, r.tier, r.storage, r.tag) == (family, shape, xpro, gpro, 'grid', 'bf16', tag)]
    return r


# one backward pass over layers of every route: a trunk layer small enough (1,024 pixels) to join wgrad_deep.hip's batch, a
# wgrad_deep.hip layer with the same batch key, the last conv on its own kernel and on the padded copy of its gradient, a 1 x 1 conv
BOOK_RUNS = [B.TRUNK_BATCH[0], _wg_run('deep', B.DEEP_WG[0], B.AFFINE_ACT, B.BNBWD), _wg_run('toimage', B.WG_THIN[0], B.ACT, B.TANH_BWD),
             _wg_run('generic', B.PADDED, B.NONE, B.TANH_BWD, 'padded'), _wg_run('generic', B.GENERIC[5], B.AFFINE_ACT, B.BNACT_BWD)]
FAMILY_KNOBS = ('SISR_TRUNK', 'SISR_DEEP', 'SISR_WGRAD_DEEP', 'SISR_THIN', 'SISR_PERSIST_MAX_WG')


def _book_gradients(E, L, monkeypatch, own_batch_slabs):
    """BOOK_RUNS through ONE engine.BackwardBook, every member prepared and handed over under the knobs of its own family
    -> [(run, case, plan, weight gradient, bias gradient)]"""
    members = []
    for r in BOOK_RUNS:
        for k in FAMILY_KNOBS:
            monkeypatch.delenv(k, raising=False)
        case, ref, p, x_op, g_op, route = _wg_setup(E, L, r, monkeypatch)
        assert route == r.family
        ref.weight.requires_grad_(True)
        ref.bias.requires_grad_(True)
        members.append((r, case, ref, p, x_op, g_op))
    book = E.BackwardBook({id(ref): p for _, _, ref, p, _, _ in members}, [m[2] for m in members], [], None, own_batch_slabs)
    before = E.KERNEL_COUNTS.get('wgrad_deep_batch', 0)
    for r, case, ref, p, x_op, g_op in members:
        for k in FAMILY_KNOBS:
            monkeypatch.delenv(k, raising=False)
        _env(monkeypatch, r.family, r.storage, r.shape)
        assert book.conv_bwd(ref, x_op, g_op, need_dgrad=False) is None
    # the two layers wgrad_deep.hip's batch keeps; the other three were launched, their slab sums wait
    assert len(book.wb.items) == 2 and len(book.wb.trunk) == 0 and len(book.wg.items) == 5
    assert [w.prep for w in book.wb.items] == [members[0][3], members[1][3]]
    for k in FAMILY_KNOBS:                             # (the batch plans its members' shares at the flush: not under SISR_WGRAD_DEEP=0)
        monkeypatch.delenv(k, raising=False)
    book.flush('final')
    assert E.KERNEL_COUNTS.get('wgrad_deep_batch', 0) == before + 1 and book.wb.items == [] and book.slabs.jobs == []
    return [(r, case, p.plans[2], book.grads[id(ref.weight)].cpu(), book.grads[id(ref.bias)].cpu()) for r, case, ref, p, _, _ in members]


def test_one_backward_book_over_every_route(E, L, monkeypatch):
    """engine.BackwardBook.conv_bwd builds ONE launch record per weight gradient and either the batch keeps it or it is launched as it
    is: members of different routes through one book, every gradient equal to its float64 reference bit for bit (grid operands, fp32
    slabs); a second book -- its batch's slab sums in the common list instead of their own -- gives the same bits"""
    first = _book_gradients(E, L, monkeypatch, True)
    for r, case, plan, gw, gb in first:
        _check_wg(r, case, gw, gb, plan)
    for (r, _, _, gw, gb), (_, _, _, gw2, gb2) in zip(first, _book_gradients(E, L, monkeypatch, False)):
        assert torch.equal(gw, gw2) and torch.equal(gb, gb2), '%r: two books differ' % r
