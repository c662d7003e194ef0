"""GPU: conv_trunk_f32.hip's tile walk and epilogue addressing at the smallest shapes that reach every path of them.

The consumer waves walk their workgroup's tiles with (n, ty, tx) advanced incrementally, run the two channel-half stages of a tile
as straight-line code, and address the tile's values with scalar offsets and immediates.  The shapes
(n, h, w[, cap]; cap = SISR_PERSIST_MAX_WG, the workgroup slots) and the statistics rows (= pixel-tile streams) each must give:

    (1, 8, 16)       1 tile, 1 stream     two stages only: the weights' second chunk is first read one barrier after the first
    (1, 16, 16, 2)   2 tiles, 1 stream    the tile loop runs exactly twice
    (1, 24, 16, 2)   3 tiles, 1 stream    odd count: the producers' staging-set swap and the last-tile exit
    (3, 24, 48, 10)  27 tiles, 5 streams  walks of 6, 6, 5, 5, 5: the stride 5 is no multiple of tiles_x = 3 or of the 9 tiles
                                          of an image, so the walk carries into rows and images at different tiles per stream
    (2, 16, 32)      8 tiles, 8 streams   every workgroup's only tile is also its last

Operands, references (F.conv2d / F.conv_transpose2d in double) and bounds are those of test_trunk_kernel_fp32_forward_role and
test_trunk_kernel_fp32_data_gradient_role in test_gpu_kernels.py: 1e-5 ('fp32': an exact fmaf chain, only the summation order
differs) and 4e-5 ('bf16x3': operands good to 2^-17) of the largest reference value; a second launch must give the same bits."""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

from gpu_helpers import FakeConv, maxrel, nchw, nhwc, pkg

pytestmark = pytest.mark.gpu

SPLIT_TOL = {'fp32': 1e-5, 'bf16x3': 4e-5}
# shape -> pixel-tile streams of a trunk launch (Cout = 64: two workgroups per stream)
WALKS = {(1, 8, 16): 1, (1, 16, 16, 2): 1, (1, 24, 16, 2): 1, (3, 24, 48, 10): 5, (2, 16, 32): 8}
WALK_SHAPES = list(WALKS)
UP_SHAPES = [(1, 8, 16), (2, 16, 32, 4)]
SLOPE = 0.2


@pytest.fixture(scope='module')
def E():
    return pkg('engine')


@pytest.fixture(scope='module')
def L():
    return pkg('_lib')


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * 2 - 1) * scale


def _walk(shape, monkeypatch):
    if len(shape) == 4:
        monkeypatch.setenv('SISR_PERSIST_MAX_WG', str(shape[3]))
    return shape[:3]


def _bc(v):
    return v[None, :, None, None]


def _merged_stats(sp, cp):
    cnt, mean_t, m2_t = cp.double().cpu(), sp[:, 0].double().cpu(), sp[:, 1].double().cpu()
    tot = cnt.sum()
    mean = (cnt[:, None] * mean_t).sum(0) / tot
    var = (m2_t + cnt[:, None] * (mean_t - mean) ** 2).sum(0) / tot
    return float(tot), mean, var


def _prep(E, wt, b, n, h, w, cout=64):
    ref = FakeConv(wt.cuda(), None if b is None else b.cuda(), E.ConvGeom(64, cout, 3, 1, 1, shuffle2=cout == 256))
    return ref, E.prepare_weights([(ref, n, h, w)], training=True)[0][0]


# ---- forward role ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fwd_case(n, h, w):
    """inputs of the forward tests and their references in double, computed once per shape"""
    x = _rand((n, 64, h, w), 131) * 2.0
    wt = _rand((64, 64, 3, 3), 132, (1.0 / 576) ** 0.5 * 1.7)
    b = _rand((64,), 133, 0.1)
    sc, sh = _rand((64,), 134) * 0.5 + 1.0, _rand((64,), 135) * 0.3
    ref = {'none': F.conv2d(x.double(), wt.double(), b.double(), padding=1),
           'affine_act': F.conv2d(F.leaky_relu(x * _bc(sc) + _bc(sh), SLOPE).double(), wt.double(), b.double(), padding=1)}
    return x, wt, b, sc, sh, ref


@pytest.mark.parametrize('precision', ['fp32', 'bf16x3'])
@pytest.mark.parametrize('pro', ['none', 'affine_act'])
@pytest.mark.parametrize('shape', WALK_SHAPES)
def test_forward_walk(E, L, shape, pro, precision, monkeypatch):
    """forward role with statistics: output against F.conv2d in double and against the generic fp32 kernel, the statistics merged
    from the per-stream rows against the reference's mean and variance; one row per stream of the walk the shape is here for"""
    tol = SPLIT_TOL[precision]
    n, h, w = _walk(shape, monkeypatch)
    x, wt, b, sc, sh, refs = _fwd_case(n, h, w)
    y_ref = refs[pro]
    slope = torch.tensor([SLOPE])
    E.set_precision(precision)
    try:
        ref, p = _prep(E, wt, b, n, h, w)
        assert not p.kinds[0]
        xd = nhwc(x).cuda()
        op = E.Operand.plain(xd) if pro == 'none' else E.Operand.affine_act(xd, sc.cuda(), sh.cuda(), slope.cuda())
        res = {}
        for sw in ('1', '0'):
            monkeypatch.setenv('SISR_TRUNK_F32CONV', sw)
            res[sw] = E.conv_forward(p, op, bias=ref.bias, stats=True)
        assert res['1'][1].shape[0] == WALKS[shape]                              # the persistent kernel took it, with this walk
        e_ref, e_gen = maxrel(nchw(res['1'][0]), y_ref), maxrel(res['1'][0], res['0'][0])
        print('forward %s %s %s: vs double %.3e, vs generic %.3e' % (shape, pro, precision, e_ref, e_gen))
        assert e_ref < tol and e_gen < tol
        t1, m1, v1 = _merged_stats(res['1'][1], res['1'][2])
        assert t1 == n * h * w
        assert maxrel(m1, y_ref.mean(dim=(0, 2, 3))) < tol and maxrel(v1, y_ref.var(dim=(0, 2, 3), unbiased=False)) < tol
        monkeypatch.setenv('SISR_TRUNK_F32CONV', '1')
        y2, sp2, cp2 = E.conv_forward(p, op, bias=ref.bias, stats=True)
        assert torch.equal(y2, res['1'][0]) and torch.equal(sp2, res['1'][1]) and torch.equal(cp2, res['1'][2])
    finally:
        E.set_precision('fp32')


@pytest.mark.parametrize('precision', ['fp32', 'bf16x3'])
@pytest.mark.parametrize('shape', WALK_SHAPES)
def test_forward_walk_through_the_deferred_finalisation(E, L, shape, precision, monkeypatch):
    """Operand.fin set to a LazyBN (as generator_engine.py does): the kernel finalises the BatchNorm of its prologue from the
    statistics rows itself, ahead of the weight fill.  The constants row it writes and the running statistics against
    E.bn_finalize on the same rows, the output against the double reference built from the tensor's own statistics and against
    the same conv on stand-alone constants"""
    tol = SPLIT_TOL[precision]
    n, h, w = _walk(shape, monkeypatch)
    x, wt, b, _, _, _ = _fwd_case(n, h, w)
    slope = torch.tensor([SLOPE])
    E.set_precision(precision)
    try:
        ref, p = _prep(E, wt, b, n, h, w)
        c1, sp, cp = E.conv_forward(p, E.Operand.plain(nhwc(x).cuda()), bias=ref.bias, stats=True)
        bn = torch.nn.BatchNorm2d(64)
        with torch.no_grad():
            bn.weight.copy_(_rand((64,), 136) * 0.5 + 1.0)
            bn.bias.copy_(_rand((64,), 137) * 0.3)
            bn.running_mean.copy_(_rand((64,), 138) * 0.2)
            bn.running_var.copy_(_rand((64,), 139) * 0.2 + 1.0)
        rm0, rv0 = bn.running_mean.double().clone(), bn.running_var.double().clone()
        bn_alone = copy.deepcopy(bn).cuda()
        bn = bn.cuda()
        k_alone = E.bn_finalize(sp, cp, bn_alone)
        y_alone, _, _ = E.conv_forward(p, E.Operand.affine_act(c1, k_alone[0], k_alone[1], slope.cuda()), bias=ref.bias, stats=True)

        def fused():
            m = copy.deepcopy(bn)
            lz = E.LazyBN(sp, cp, m)
            op = E.Operand.affine_act(c1, lz.k[0], lz.k[1], slope.cuda())
            op.fin = lz
            out = E.conv_forward(p, op, bias=ref.bias, stats=True)
            assert lz.done and out[1].shape[0] == WALKS[shape]                   # finalised by the conv, on the persistent kernel
            return out, lz.k, m

        (y, sp2, cp2), k, m = fused()
        # the reference in double from the first conv's output as stored
        c = nchw(c1).double().cpu()
        mean, var = c.mean(dim=(0, 2, 3)), c.var(dim=(0, 2, 3), unbiased=False)
        invstd = 1.0 / torch.sqrt(var + 1e-5)
        g64, b64 = bn_alone.weight.double().cpu(), bn_alone.bias.double().cpu()
        k_ref = torch.stack([g64 * invstd, b64 - mean * g64 * invstd, mean, invstd])
        y_ref = F.conv2d(F.leaky_relu(c * _bc(k_ref[0]) + _bc(k_ref[1]), SLOPE), wt.double(), b.double(), padding=1)
        for row in range(4):
            e_a, e_r = maxrel(k[row], k_alone[row]), maxrel(k[row], k_ref[row])
            print('fin %s %s k[%d]: vs bn_finalize %.3e, vs double %.3e' % (shape, precision, row, e_a, e_r))
            assert e_a < tol and e_r < tol
        assert maxrel(m.running_mean, bn_alone.running_mean) < tol and maxrel(m.running_var, bn_alone.running_var) < tol
        cnt = n * h * w
        assert maxrel(m.running_mean, 0.9 * rm0 + 0.1 * mean) < tol                 # momentum 0.1, unbiased variance
        assert maxrel(m.running_var, 0.9 * rv0 + 0.1 * var * cnt / (cnt - 1)) < tol
        e_ref, e_alone = maxrel(nchw(y), y_ref), maxrel(y, y_alone)
        print('fin %s %s: vs double %.3e, vs stand-alone constants %.3e' % (shape, precision, e_ref, e_alone))
        assert e_ref < tol and e_alone < tol
        _, m1, v1 = _merged_stats(sp2, cp2)
        assert maxrel(m1, y_ref.mean(dim=(0, 2, 3))) < tol and maxrel(v1, y_ref.var(dim=(0, 2, 3), unbiased=False)) < tol
        (y_b, sp_b, _), k_b, _ = fused()
        assert torch.equal(y_b, y) and torch.equal(k_b, k) and torch.equal(sp_b, sp2)
    finally:
        E.set_precision('fp32')


@pytest.mark.parametrize('precision', ['fp32', 'bf16x3'])
@pytest.mark.parametrize('res_slope', [None, 0.25])
@pytest.mark.parametrize('shape', WALK_SHAPES)
def test_skip_sum_walk(E, L, shape, res_slope, precision, monkeypatch):
    """skip-sum prologue: conv(lrelu(res) + (scale * t + shift)) with the sum stored once by the staging waves -- the materialised
    sum bit-identical to the elementwise pass, output and statistics bit-identical to the plain conv on that sum (same kernel,
    same staged values), and the output against F.conv2d in double"""
    tol = SPLIT_TOL[precision]
    n, h, w = _walk(shape, monkeypatch)
    rs, t = _rand((n, 64, h, w), 171) * 2.0, _rand((n, 64, h, w), 172) * 2.0
    sc, sh = _rand((64,), 173) * 0.5 + 1.0, _rand((64,), 174) * 0.3
    wt = _rand((64, 64, 3, 3), 175, (1.0 / 576) ** 0.5 * 1.7)
    b = _rand((64,), 176, 0.1)
    lhs = rs if res_slope is None else F.leaky_relu(rs, res_slope)
    y_ref = F.conv2d((lhs + (_bc(sc) * t + _bc(sh))).double(), wt.double(), b.double(), padding=1)
    E.set_precision(precision)
    try:
        resid, td = nhwc(rs).cuda(), nhwc(t).cuda()
        slope = None if res_slope is None else torch.tensor([res_slope], device='cuda')
        ref, p = _prep(E, wt, b, n, h, w)
        assert E.trunk_takes_skip_sum(p, resid, td)
        out = torch.full_like(resid, float('nan'))
        y1, sp1, cp1 = E.conv_forward(p, E.Operand.res_affine(resid, slope, td, sc.cuda(), sh.cuda(), out), bias=ref.bias, stats=True)
        assert sp1.shape[0] == WALKS[shape]
        summed = E.eltwise_res_affine(resid, slope, td, sc.cuda(), sh.cuda())
        y0, sp0, cp0 = E.conv_forward(p, E.Operand.plain(summed), bias=ref.bias, stats=True)
        assert torch.equal(out, summed)
        assert torch.equal(y1, y0) and torch.equal(sp1, sp0) and torch.equal(cp1, cp0)
        e_ref = maxrel(nchw(y1), y_ref)
        print('skip sum %s %s %s: vs double %.3e' % (shape, res_slope, precision, e_ref))
        assert e_ref < tol
    finally:
        E.set_precision('fp32')


# ---- data-gradient role ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dgrad_case(n, h, w):
    g_in, c = _rand((n, 64, h, w), 141), _rand((n, 64, h, w), 142) * 2.0
    wt = _rand((64, 64, 3, 3), 143, (1.0 / 576) ** 0.5 * 1.7)
    qa, qb, qd = _rand((64,), 144) * 0.3 + 1.0, _rand((64,), 145) * 0.2, _rand((64,), 146) * 0.1
    ks, kt = _rand((64,), 147) * 0.5 + 1.0, _rand((64,), 148) * 0.3
    skip = _rand((n, 64, h, w), 149)
    xb = _rand((n, 64, h, w), 160) * 2.0
    gamma, beta = _rand((64,), 161) + 1.5, _rand((64,), 162)
    out = {}
    for pro in ('bnbwd', 'bnact_bwd'):
        gg = g_in if pro == 'bnbwd' else torch.where(_bc(ks) * c + _bc(kt) > 0, g_in, SLOPE * g_in)
        dy = _bc(qa) * gg + _bc(qb) * c + _bc(qd)
        out[pro] = F.conv_transpose2d(dy.double(), wt.double(), padding=1)
    return g_in, c, wt, (qa, qb, qd), (ks, kt), skip, xb, gamma, beta, out


@pytest.mark.parametrize('precision', ['fp32', 'bf16x3'])
@pytest.mark.parametrize('pro,res,bnb', [('bnbwd', False, None), ('bnbwd', True, 'plain'), ('bnact_bwd', True, 'act'),
                                         ('bnact_bwd', False, 'plain'), ('bnact_bwd', True, None), ('bnbwd', False, 'act')])
@pytest.mark.parametrize('shape', WALK_SHAPES)
def test_data_gradient_walk(E, L, shape, pro, res, bnb, precision, monkeypatch):
    """data-gradient role: BatchNorm-backward prologues, skip gradient added in the epilogue, and the fused rows of the next
    BatchNorm's backward reductions: sum(g), sum(g xhat) per channel and the slope term against sums of the stored gradient in
    double, and finalized against the stand-alone reduction (2e-5, as test_trunk_kernel_fp32_fused_bn_backward_reductions)"""
    tol = SPLIT_TOL[precision]
    n, h, w = _walk(shape, monkeypatch)
    g_in, c, wt, (qa, qb, qd), (ks, kt), skip, xb, gamma, beta, refs = _dgrad_case(n, h, w)
    out_ref = refs[pro] + (skip.double() if res else 0.0)
    slope = torch.tensor([SLOPE])
    mean = xb.mean(dim=(0, 2, 3))
    invstd = torch.rsqrt(xb.var(dim=(0, 2, 3), unbiased=False) + 1e-5)
    kb = torch.stack([gamma * invstd, beta - mean * gamma * invstd, mean, invstd])
    E.set_precision(precision)
    try:
        ref, p = _prep(E, wt, None, n, h, w)
        assert E.can_fuse_bn_backward(p)                                         # the persistent kernel takes this geometry
        gd, cd = nhwc(g_in).cuda(), nhwc(c).cuda()
        kw = dict(pa=qa.cuda(), pb=qb.cuda(), pd=qd.cuda())
        if pro == 'bnact_bwd':
            kw.update(ps=ks.cuda(), pt=kt.cuda(), slope=slope.cuda())
        op = E.Operand(gd, tuple(cd.shape), pro=L.PRO_BNACT_BWD if pro == 'bnact_bwd' else L.PRO_BNBWD, x2=cd, **kw)
        rd = nhwc(skip).cuda() if res else None
        xd, kbd = nhwc(xb).cuda(), kb.cuda()
        b_slope = slope.cuda() if bnb == 'act' else None

        def run():
            if bnb is None:
                return E.conv_dgrad(p, op, res=rd), None
            return E.conv_dgrad(p, op, res=rd, bnb=(xd, kbd, b_slope))

        g, part = run()
        monkeypatch.setenv('SISR_TRUNK_F32CONV', '0')
        g_gen = E.conv_dgrad(p, op, res=rd)
        monkeypatch.setenv('SISR_TRUNK_F32CONV', '1')
        e_ref, e_gen = maxrel(nchw(g), out_ref), maxrel(g, g_gen)
        print('dgrad %s %s res=%s %s: vs double %.3e, vs generic %.3e' % (shape, pro, res, precision, e_ref, e_gen))
        assert e_ref < tol and e_gen < tol
        if res:
            assert torch.equal(rd, nhwc(skip).cuda())
        if bnb is not None:
            assert part is not None and part.shape[0] == 2 * WALKS[shape]         # one row per workgroup of the walk
            g64, x64 = nchw(g).double().cpu(), xb.double()
            if bnb == 'act':
                z = _bc(kb[0].double()) * x64 + _bc(kb[1].double())
                neg = ~(z > 0)
                s_slope = float((g64 * z)[neg].sum())
                g64 = torch.where(neg, g64 * SLOPE, g64)
            xhat = (x64 - _bc(kb[2].double())) * _bc(kb[3].double())
            sums = part.double().sum(0).cpu()
            e1, e2 = maxrel(sums[:64], g64.sum(dim=(0, 2, 3))), maxrel(sums[64:128], (g64 * xhat).sum(dim=(0, 2, 3)))
            print('dgrad %s bnb=%s %s: sum(g) %.3e, sum(g xhat) %.3e' % (shape, bnb, precision, e1, e2))
            assert e1 < 2e-5 and e2 < 2e-5
            if bnb == 'act':
                assert abs(float(sums[128]) - s_slope) < 2e-5 * max(1.0, abs(s_slope))
            fused = E.bn_backward(g, xd, kbd, gamma.cuda(), slope=b_slope, part=part)
            plain = E.bn_backward(g, xd, kbd, gamma.cuda(), slope=b_slope)
            for a_, b_ in zip(fused, plain):
                if a_ is not None:
                    assert maxrel(a_, b_) < 2e-5
        g2, part2 = run()
        assert torch.equal(g2, g) and (part is None or torch.equal(part2, part))
    finally:
        E.set_precision('fp32')


# ---- the upscale conv: PixelShuffle store, four-launch data gradient ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _up_case(n, h, w):
    x = _rand((n, 64, h, w), 281) * 2.0
    wt = _rand((256, 64, 3, 3), 282, (1.0 / 576) ** 0.5 * 1.7)
    b = _rand((256,), 283, 0.1)
    sc, sh = _rand((64,), 284) * 0.5 + 1.0, _rand((64,), 285) * 0.3
    ref = {'none': F.pixel_shuffle(F.conv2d(x.double(), wt.double(), b.double(), padding=1), 2),
           'affine_act': F.pixel_shuffle(F.conv2d(F.leaky_relu(x * _bc(sc) + _bc(sh), 0.25).double(), wt.double(), b.double(),
                                                  padding=1), 2)}
    # data gradient: autograd through conv (no bias) -> pixel_shuffle -> PReLU
    xg = x.double().requires_grad_(True)
    pre_ref = F.pixel_shuffle(F.conv2d(xg, wt.double(), None, padding=1), 2)
    pre = pre_ref.detach().float()
    g = _rand((n, 64, 2 * h, 2 * w), 304)
    pre_ref.backward(torch.where(pre > 0, g, 0.25 * g).double())
    skip = _rand((n, 64, h, w), 303)
    return x, wt, b, sc, sh, ref, pre, g, skip, xg.grad


@pytest.mark.parametrize('precision', ['fp32', 'bf16x3'])
@pytest.mark.parametrize('pro', ['none', 'affine_act'])
@pytest.mark.parametrize('shape', UP_SHAPES)
def test_upscale_forward_walk(E, L, shape, pro, precision, monkeypatch):
    """forward role with Cout = 256 stored through PixelShuffle(2): the shuffled tile's column stride does not fit the store's
    immediate for columns 8 .. 11 -- against F.pixel_shuffle(F.conv2d(...)) in double and the generic kernel"""
    tol = SPLIT_TOL[precision]
    n, h, w = _walk(shape, monkeypatch)
    x, wt, b, sc, sh, refs, _, _, _, _ = _up_case(n, h, w)
    slope = torch.tensor([0.25])
    E.set_precision(precision)
    try:
        ref, p = _prep(E, wt, b, n, h, w, cout=256)
        assert not p.kinds[0]
        xd = nhwc(x).cuda()
        op = E.Operand.plain(xd) if pro == 'none' else E.Operand.affine_act(xd, sc.cuda(), sh.cuda(), slope.cuda())
        out = {}
        for sw in ('1', '0'):
            monkeypatch.setenv('SISR_TRUNK_UP', sw)
            out[sw] = E.conv_forward(p, op, bias=ref.bias)[0]
        assert tuple(out['1'].shape) == (n, 2 * h, 2 * w, 64)
        e_ref, e_gen = maxrel(nchw(out['1']), refs[pro]), maxrel(out['1'], out['0'])
        print('upscale forward %s %s %s: vs double %.3e, vs generic %.3e' % (shape, pro, precision, e_ref, e_gen))
        assert e_ref < tol and e_gen < tol
        assert not torch.equal(out['1'], out['0'])                               # (two kernels: the persistent one did run)
        monkeypatch.setenv('SISR_TRUNK_UP', '1')
        assert torch.equal(E.conv_forward(p, op, bias=ref.bias)[0], out['1'])
    finally:
        E.set_precision('fp32')


@pytest.mark.parametrize('precision', ['fp32', 'bf16x3'])
@pytest.mark.parametrize('res', [False, True])
@pytest.mark.parametrize('shape', UP_SHAPES)
def test_upscale_data_gradient_walk(E, L, shape, res, precision, monkeypatch):
    """data gradient of the upscale conv: four launches of the data-gradient role, one per PixelShuffle phase, each adding onto
    the one before through the epilogue's residual read -- against autograd in double and the generic kernel"""
    tol = SPLIT_TOL[precision]
    n, h, w = _walk(shape, monkeypatch)
    _, wt, _, _, _, _, pre, g, skip, gx = _up_case(n, h, w)
    want = gx + (skip.double() if res else 0.0)
    slope = torch.tensor([0.25])
    E.set_precision(precision)
    try:
        ref, p = _prep(E, wt, None, n, h, w, cout=256)
        gd, pd_ = nhwc(g).cuda(), nhwc(pre).cuda()
        dy_op = E.Operand(gd, (n, h, w, 256), pro=L.PRO_ACT_BWD, mode=L.X_UNSHUFFLE2, x2=pd_, slope=slope.cuda())
        rd = nhwc(skip).cuda() if res else None
        out = {}
        for sw in ('1', '0'):
            monkeypatch.setenv('SISR_TRUNK_UP', sw)
            out[sw] = E.conv_dgrad(p, dy_op, res=rd)
        assert tuple(out['1'].shape) == (n, h, w, 64)
        e_ref, e_gen = maxrel(nchw(out['1']), want), maxrel(out['1'], out['0'])
        print('upscale dgrad %s res=%s %s: vs double %.3e, vs generic %.3e' % (shape, res, precision, e_ref, e_gen))
        assert e_ref < tol and e_gen < tol
        assert not torch.equal(out['1'], out['0'])
        if res:
            assert torch.equal(rd, nhwc(skip).cuda())
        monkeypatch.setenv('SISR_TRUNK_UP', '1')
        assert torch.equal(E.conv_dgrad(p, dy_op, res=rd), out['1'])
    finally:
        E.set_precision('fp32')
