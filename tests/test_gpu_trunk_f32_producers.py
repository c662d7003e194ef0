"""GPU: the staging (producer) waves of conv_trunk_f32.hip at the smallest shapes that reach what test_gpu_trunk_f32_walk.py's do not.

The producers walk their workgroup's tiles with (n, ty, tx) advanced incrementally, keep what depends on the tile alone (item
addresses, edge test, the lane masks of the items outside the image) from one channel-half stage to the next, hold one staging
register set per channel half, and -- in the skip-sum role -- store the materialised sum half by the workgroup of cout half 0 and
half by its partner.  All interior tiles of the walk test's (3, 24, 48, 10) fall on even walk positions.  The shapes here
(n, h, w, cap; cap = SISR_PERSIST_MAX_WG, the workgroup slots):

    (1, 24, 64, 2)   12 tiles, 1 stream, tiles_x = 4   interior tiles at walk positions 5 and 6 (odd and even), edge -> interior
                                                       -> edge in both directions
    (2, 24, 48, 4)   18 tiles, 2 streams of 9          the incremental walk (stride 2 over rows of 3 and images of 9 tiles)
                                                       carries into the next row and image at different tiles per stream

Operands, references (F.conv2d / F.conv_transpose2d in double) and bounds are those of the walk test: 1e-5 ('fp32') and 4e-5
('bf16x3') of the largest reference value; a second launch must give the same bits.  The materialised sum of the skip-sum role
is held to what the kernel gave before its store was shared between the two workgroups: bit-identical to the stand-alone
elementwise pass (test_skip_sum_walk asserts the same for its shapes)."""
import functools

import pytest
import torch
import torch.nn.functional as F

from gpu_helpers import FakeConv, maxrel, nchw, nhwc, pkg

pytestmark = pytest.mark.gpu

SPLIT_TOL = {'fp32': 1e-5, 'bf16x3': 4e-5}
# shape -> pixel-tile streams of a trunk launch (Cout = 64: two workgroups per stream)
WALKS = {(1, 24, 64, 2): 1, (2, 24, 48, 4): 2}
SHAPES = list(WALKS)
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


def _bc(v):
    return v[None, :, None, None]


def _prep(E, wt, b, n, h, w):
    ref = FakeConv(wt.cuda(), None if b is None else b.cuda(), E.ConvGeom(64, 64, 3, 1, 1))
    return ref, E.prepare_weights([(ref, n, h, w)], training=True)[0][0]


@functools.lru_cache(maxsize=None)
def _weights():
    return _rand((64, 64, 3, 3), 132, (1.0 / 576) ** 0.5 * 1.7), _rand((64,), 133, 0.1)


# ---- forward role ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fwd_case(n, h, w, slope):
    x = _rand((n, 64, h, w), 131) * 2.0
    wt, b = _weights()
    sc, sh = _rand((64,), 134) * 0.5 + 1.0, _rand((64,), 135) * 0.3
    y_ref = F.conv2d(F.leaky_relu(x * _bc(sc) + _bc(sh), slope).double(), wt.double(), b.double(), padding=1)
    return x, sc, sh, y_ref


def _forward(E, shape, slope_v, precision, monkeypatch):
    tol = SPLIT_TOL[precision]
    n, h, w, cap = shape
    monkeypatch.setenv('SISR_PERSIST_MAX_WG', str(cap))
    x, sc, sh, y_ref = _fwd_case(n, h, w, slope_v)
    wt, b = _weights()
    E.set_precision(precision)
    try:
        ref, p = _prep(E, wt, b, n, h, w)
        op = E.Operand.affine_act(nhwc(x).cuda(), sc.cuda(), sh.cuda(), torch.tensor([slope_v]).cuda())
        res = {}
        for sw in ('1', '0'):
            monkeypatch.setenv('SISR_TRUNK_F32CONV', sw)
            res[sw] = E.conv_forward(p, op, bias=ref.bias, stats=True)
        assert res['1'][1].shape[0] == WALKS[shape]                              # the persistent kernel took it, with this walk
        e_ref, e_gen = maxrel(nchw(res['1'][0]), y_ref), maxrel(res['1'][0], res['0'][0])
        print('forward %s slope %s %s: vs double %.3e, vs generic %.3e' % (shape, slope_v, precision, e_ref, e_gen))
        assert e_ref < tol and e_gen < tol
        monkeypatch.setenv('SISR_TRUNK_F32CONV', '1')
        y2, sp2, cp2 = E.conv_forward(p, op, bias=ref.bias, stats=True)
        assert torch.equal(y2, res['1'][0]) and torch.equal(sp2, res['1'][1]) and torch.equal(cp2, res['1'][2])
    finally:
        E.set_precision('fp32')


@pytest.mark.parametrize('precision', ['fp32', 'bf16x3'])
@pytest.mark.parametrize('shape', SHAPES)
def test_forward_role(E, shape, precision, monkeypatch):
    """BatchNorm-apply + leaky ReLU prologue (slope inside [0, 1]: max(v, slope v)) against F.conv2d in double and the generic kernel"""
    _forward(E, shape, SLOPE, precision, monkeypatch)


@pytest.mark.parametrize('precision', ['fp32', 'bf16x3'])
def test_forward_role_slope_outside_unit_interval(E, precision, monkeypatch):
    """slope 1.5: max(v, slope v) is not the leaky ReLU -- the walk's compare-and-select instance"""
    _forward(E, SHAPES[0], 1.5, precision, monkeypatch)


# ---- skip-sum role ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sum_case(n, h, w):
    rs, t = _rand((n, 64, h, w), 171) * 2.0, _rand((n, 64, h, w), 172) * 2.0
    sc, sh = _rand((64,), 173) * 0.5 + 1.0, _rand((64,), 174) * 0.3
    wt, b = _weights()
    y_ref = F.conv2d((F.leaky_relu(rs, 0.25) + (_bc(sc) * t + _bc(sh))).double(), wt.double(), b.double(), padding=1)
    return rs, t, sc, sh, y_ref


@pytest.mark.parametrize('precision', ['fp32', 'bf16x3'])
@pytest.mark.parametrize('shape', SHAPES)
def test_skip_sum_role(E, shape, precision, monkeypatch):
    """conv(lrelu(res) + (scale * t + shift)): output against F.conv2d in double; output and statistics bit-identical to the plain
    conv on the materialised sum (same kernel, same staged values); a second launch gives the same bits"""
    tol = SPLIT_TOL[precision]
    n, h, w, cap = shape
    monkeypatch.setenv('SISR_PERSIST_MAX_WG', str(cap))
    rs, t, sc, sh, y_ref = _sum_case(n, h, w)
    wt, b = _weights()
    E.set_precision(precision)
    try:
        resid, td = nhwc(rs).cuda(), nhwc(t).cuda()
        slope = torch.tensor([0.25], device='cuda')
        ref, p = _prep(E, wt, b, n, h, w)
        assert E.trunk_takes_skip_sum(p, resid, td)
        out = torch.full_like(resid, float('nan'))
        y1, sp1, cp1 = E.conv_forward(p, E.Operand.res_affine(resid, slope, td, sc.cuda(), sh.cuda(), out), bias=ref.bias, stats=True)
        assert sp1.shape[0] == WALKS[shape]
        y0, sp0, cp0 = E.conv_forward(p, E.Operand.plain(out), bias=ref.bias, stats=True)
        assert torch.equal(y1, y0) and torch.equal(sp1, sp0) and torch.equal(cp1, cp0)
        e_ref = maxrel(nchw(y1), y_ref)
        print('skip sum %s %s: vs double %.3e' % (shape, precision, e_ref))
        assert e_ref < tol
        out2 = torch.full_like(resid, float('nan'))
        y2, sp2, _ = E.conv_forward(p, E.Operand.res_affine(resid, slope, td, sc.cuda(), sh.cuda(), out2), bias=ref.bias, stats=True)
        assert torch.equal(y2, y1) and torch.equal(sp2, sp1) and torch.equal(out2, out)
    finally:
        E.set_precision('fp32')


@pytest.mark.parametrize('precision', ['fp32', 'bf16x3'])
@pytest.mark.parametrize('cap', [None, 2])
@pytest.mark.parametrize('shape', [(1, 8, 16)] + [s[:3] for s in SHAPES])
def test_skip_sum_store_is_complete(E, shape, cap, precision, monkeypatch):
    """the materialised sum, stored half by each workgroup of a cout pair into a tensor of NaNs: no NaN is left, and every value
    carries the bits of the stand-alone elementwise pass -- with the default grid (one tile per workgroup at these sizes) and
    with one stream walking all tiles"""
    n, h, w = shape
    if cap is not None:
        monkeypatch.setenv('SISR_PERSIST_MAX_WG', str(cap))
    rs, t, sc, sh, _ = _sum_case(n, h, w)
    wt, b = _weights()
    E.set_precision(precision)
    try:
        resid, td = nhwc(rs).cuda(), nhwc(t).cuda()
        slope = torch.tensor([0.25], device='cuda')
        ref, p = _prep(E, wt, b, n, h, w)
        assert E.trunk_takes_skip_sum(p, resid, td)
        out = torch.full_like(resid, float('nan'))
        _, sp, _ = E.conv_forward(p, E.Operand.res_affine(resid, slope, td, sc.cuda(), sh.cuda(), out), bias=ref.bias, stats=True)
        tiles = n * (h // 8) * (w // 16)
        assert sp.shape[0] == (tiles if cap is None else 1)                      # the persistent kernel took it, with this grid
        summed = E.eltwise_res_affine(resid, slope, td, sc.cuda(), sh.cuda())
        left = int(torch.isnan(out).sum())
        print('skip-sum store %s cap %s %s: NaN left %d' % (shape, cap, precision, left))
        assert left == 0
        assert torch.equal(out, summed)
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
    out = {}
    for pro in ('bnbwd', 'bnact_bwd'):
        gg = g_in if pro == 'bnbwd' else torch.where(_bc(ks) * c + _bc(kt) > 0, g_in, SLOPE * g_in)
        dy = _bc(qa) * gg + _bc(qb) * c + _bc(qd)
        out[pro] = F.conv_transpose2d(dy.double(), wt.double(), padding=1)
    return g_in, c, wt, (qa, qb, qd), (ks, kt), skip, out


@pytest.mark.parametrize('precision', ['fp32', 'bf16x3'])
@pytest.mark.parametrize('pro,res', [('bnbwd', False), ('bnact_bwd', True)])
@pytest.mark.parametrize('shape', SHAPES)
def test_data_gradient_roles(E, L, shape, pro, res, precision, monkeypatch):
    """BatchNorm-backward prologues (two staged tensors per item) against F.conv_transpose2d in double and the generic kernel"""
    tol = SPLIT_TOL[precision]
    n, h, w, cap = shape
    monkeypatch.setenv('SISR_PERSIST_MAX_WG', str(cap))
    g_in, c, wt, (qa, qb, qd), (ks, kt), skip, refs = _dgrad_case(n, h, w)
    out_ref = refs[pro] + (skip.double() if res else 0.0)
    E.set_precision(precision)
    try:
        ref, p = _prep(E, wt, None, n, h, w)
        assert E.can_fuse_bn_backward(p)                                         # the persistent kernel takes this geometry
        gd, cd = nhwc(g_in).cuda(), nhwc(c).cuda()
        kw = dict(pa=qa.cuda(), pb=qb.cuda(), pd=qd.cuda())
        if pro == 'bnact_bwd':
            kw.update(ps=ks.cuda(), pt=kt.cuda(), slope=torch.tensor([SLOPE]).cuda())
        op = E.Operand(gd, tuple(cd.shape), pro=L.PRO_BNACT_BWD if pro == 'bnact_bwd' else L.PRO_BNBWD, x2=cd, **kw)
        rd = nhwc(skip).cuda() if res else None
        g = E.conv_dgrad(p, op, res=rd)
        monkeypatch.setenv('SISR_TRUNK_F32CONV', '0')
        g_gen = E.conv_dgrad(p, op, res=rd)
        monkeypatch.setenv('SISR_TRUNK_F32CONV', '1')
        e_ref, e_gen = maxrel(nchw(g), out_ref), maxrel(g, g_gen)
        print('dgrad %s %s res=%s %s: vs double %.3e, vs generic %.3e' % (shape, pro, res, precision, e_ref, e_gen))
        assert e_ref < tol and e_gen < tol
        assert torch.equal(E.conv_dgrad(p, op, res=rd), g)
    finally:
        E.set_precision('fp32')
