"""GPU: value tests of the weight-side kernels (csrc/spectral.hip) -- the spectral-norm power iteration, the weight-gradient
epilogue (generic and fast path) and multi-entry packing -- one entry point at a time through the C ABI, against float64.

The discipline of tests/test_gpu_glue.py: every output (u, v, u_used, v_used, sigma[2], sn_work, grad, grad_bias, dot_work) lives
between sentinel guards that must be intact afterwards; every launch runs twice from the same pre-fill (u and v restored: the kernel
updates them in place) and must give identical bits; bounds come from the number formats and the kernels' chain lengths
(tests/weights_cases.py holds the inputs, the float64 references and the derivation of every bound; u = 2^-24).

a. sisr_weights_sn: one legacy spectral_norm step, checked stage by stage (t = W^T u, v, u, sigma; sigma[1] = fl(1 / sigma[0]) and
   u_used / v_used bit-exact), every weight alone and all of them in one table beside an entry without u and one in evaluation
   mode; the table run must reproduce the single runs bit for bit (the reduction order of a weight does not depend on the grid).
b. sisr_weights_grad / sisr_weights_grad_fast: a synthetic reduced slab (no convolution), NaN in every padding slot,
   (G - (<G, W_orig> / sigma) u v^T) / sigma with the rank-one term half the size of G (rho, asserted >= 0.25).
c. sisr_weights_pack / sisr_weights_pack_deep through engine.prepare_weights: the images of a six-layer table are bit-identical
   to the images each layer gets alone (the conv tests validate a single-entry image functionally)."""
import ctypes as C

import numpy as np
import pytest
import torch

import weights_cases as WC
from gpu_helpers import SENT, Buf, FakeConv, _bits, assert_within, pkg, run2

pytestmark = pytest.mark.gpu
F32 = torch.float32


@pytest.fixture(scope='module')
def L():
    return pkg('_lib')


@pytest.fixture(scope='module')
def E():
    return pkg('engine')


def _st():
    return torch.cuda.current_stream().cuda_stream


def _table(E, table):
    return E._table_to_device(table, torch.device('cuda'))


def _same_bits(a, b):
    return torch.equal(_bits(a.contiguous()), _bits(b.contiguous()))


class Seeded(Buf):
    """a Buf whose body holds `init` before every launch (u and v: inputs the kernel updates in place)"""

    def __init__(self, init):
        self.init = init.to(F32).contiguous().cuda()
        super().__init__(init.numel())

    def reset(self):
        self.whole.fill_(SENT)
        self.body.copy_(self.init)


def _sid(shape):
    return 'x'.join(str(d) for d in shape)


def _untouched(buf):
    return bool((buf.body == SENT).all())


# ---- a. power iteration ---------------------------------------------------------------------------------------------------------
# rows x cols and the branch each shape reaches (SN_RB = 16 rows per block, SN_CB = 1024 columns per block, 4 rows per sn_w_v
# workgroup with a 12-deep load round of 768 columns, 256 threads in the finishing kernel):
#   (64, 32, 3)    64 x 288   baseline: four whole row blocks on the float4 path
#   (40, 24, 3)    40 x 216   float4 path for two row blocks, the scalar path for the ragged third (8 rows)
#   (64, 3, 3)     64 x 27    cols & 3 != 0: scalar path
#   (16, 3, 9)     16 x 243   cols & 3 != 0: scalar path, one row block
#   (3, 64, 3)      3 x 576   fewer rows than one sn_w_v workgroup serves
#   (32, 96, 3)    32 x 864   second load round of sn_w_v with a clamped tail (864 = 768 + 96)
#   (48, 128, 3)   48 x 1152  second column block (128 of its 1024 columns used)
#   (272, 32, 1)  272 x 32    rows > 256: second trip of the finishing kernel's strided loops
#   (20, 1, 3)     20 x 9     cols = 9
class SnEntry:
    def __init__(self, shape, seed=0, init=None):
        self.shape = shape
        self.w, self.u_in, self.v_in = WC.sn_inputs(shape, seed)
        if init is not None:
            self.u_in, self.v_in = init
        self.rows, self.cols = self.w.shape
        self.wd = self.w.contiguous().cuda()
        self.u, self.v = Seeded(self.u_in), Seeded(self.v_in)
        self.u_used, self.v_used = Buf(self.rows), Buf(self.cols)
        self.sigma = Buf(2)
        self.sn_work = Buf(WC.sn_work_floats(self.rows, self.cols))
        self.outs = [self.u, self.v, self.u_used, self.v_used, self.sigma, self.sn_work]

    def fill(self, t, training=1, with_u=True):
        cout, cin, k = self.shape
        t.w_orig, t.u, t.v = self.wd.data_ptr(), (self.u.ptr() if with_u else None), self.v.ptr()
        t.u_used, t.v_used, t.sigma, t.sn_work = self.u_used.ptr(), self.v_used.ptr(), self.sigma.ptr(), self.sn_work.ptr()
        t.Cout, t.Cin, t.KH, t.KW, t.training = cout, cin, k, k, training

    def results(self):
        return {n: getattr(self, n).cpu() for n in ('u', 'v', 'u_used', 'v_used', 'sigma', 'sn_work')}


def _run_sn(L, E, entries, flags=None):
    """one table, run2 over every entry's outputs -> the device table (kept alive by the caller)"""
    table = (L.WeightDesc * len(entries))()
    for i, e in enumerate(entries):
        e.fill(table[i], *(flags[i] if flags else ()))
    tab = _table(E, table)
    max_rows, max_cols = max(e.rows for e in entries), max(e.cols for e in entries)
    run2(lambda: L.lib().sisr_weights_sn(tab.data_ptr(), len(entries), max_rows, max_cols, _st()), [o for e in entries for o in e.outs])
    return tab, max_rows, max_cols


def _check_sn(e, got, training, what):
    """got: results() of a run; stage-by-stage comparison as laid out in weights_cases.sn_reference"""
    rows, cols = e.rows, e.cols
    nrb = WC.cdiv(rows, WC.SN_RB)
    ref = WC.sn_reference(e.w, e.u_in, got['v'], got['u'], training)
    work = got['sn_work']
    if training:
        assert_within(work[:cols], *ref['t'], what + ' t = W^T u')
        assert_within(got['v'], *ref['v'], what + ' v')
        assert_within(got['u'], *ref['u'], what + ' u')
    else:
        assert _same_bits(got['u'], e.u_in) and _same_bits(got['v'], e.v_in), what + ': evaluation mode changed u or v'
        assert bool((work[:nrb * cols] == SENT).all()), what + ': evaluation mode wrote the W^T u scratch'
    # the rows' dots as the kernel left them in the scratch (not yet scaled by 1 / |t| when training): the tightest view of sn_w_v
    s_raw = work[nrb * cols:]
    assert_within(s_raw, *WC.sn_rows_dot(e.w, work[:cols] if training else e.v_in), what + (' W t' if training else ' W v'))
    if not training:
        assert_within(got['sigma'][:1], *WC.sn_sigma_from_rows(got['u'], s_raw), what + ' sigma from the rows')
    assert_within(got['sigma'][:1], *ref['sigma'], what + ' sigma')
    s0 = np.float32(got['sigma'][0].item())
    assert np.float32(got['sigma'][1].item()).tobytes() == (np.float32(1) / s0).tobytes(), what + ': sigma[1] != fl(1 / sigma[0])'
    assert _same_bits(got['u_used'], got['u']) and _same_bits(got['v_used'], got['v']), what + ': u_used / v_used'


_SN_ALONE = {}


def _sn_alone(L, E, shape):
    """the shape alone in its table (computed once, shared with the table test): results of the first and of a second call"""
    if shape not in _SN_ALONE:
        e = SnEntry(shape)
        tab, mr, mc = _run_sn(L, E, [e])
        first = e.results()
        assert L.lib().sisr_weights_sn(tab.data_ptr(), 1, mr, mc, _st()) == 0          # continues from the first call's u, v
        torch.cuda.synchronize()
        assert all(o.guards_intact() for o in e.outs)
        _SN_ALONE[shape] = (e, first, e.results())
    return _SN_ALONE[shape]


@pytest.mark.parametrize('shape', WC.SN_SHAPES, ids=_sid)
def test_sn_each_weight_alone(L, E, shape):
    e, first, second = _sn_alone(L, E, shape)
    _check_sn(e, first, 1, 'sn %s alone' % (shape,))
    # a second call continues from the first call's u and v: the same bits as a fresh step started from them
    e2 = SnEntry(shape, init=(first['u'], first['v']))
    _run_sn(L, E, [e2])
    got2 = e2.results()
    _check_sn(e2, got2, 1, 'sn %s second step' % (shape,))
    for n in ('u', 'v', 'u_used', 'v_used', 'sigma'):
        assert _same_bits(second[n], got2[n]), 'second call: %s' % n


def test_sn_table_with_null_u_and_evaluation_entries(L, E):
    """all nine weights in one table (max_rows = 272 and max_cols = 1152 come from different entries, so every weight runs in a
    grid sized by others) + an entry without u (sigma exactly [1, 1], nothing else written) + an entry in evaluation mode"""
    entries = [SnEntry(s) for s in WC.SN_SHAPES]
    flags = [(1, True)] * len(entries)
    null_u, evl = SnEntry((40, 24, 3), seed=1), SnEntry((32, 96, 3), seed=2)
    entries[3:3] = [null_u]
    flags[3:3] = [(1, False)]
    entries[7:7] = [evl]
    flags[7:7] = [(0, True)]
    _, max_rows, max_cols = _run_sn(L, E, entries, flags)
    assert (max_rows, max_cols) == (272, 1152)
    for e in entries:
        got = e.results()
        what = 'sn %s in the table' % (e.shape,)
        if e is null_u:
            assert got['sigma'].tolist() == [1.0, 1.0], got['sigma']
            assert _same_bits(got['u'], e.u_in) and _same_bits(got['v'], e.v_in)
            assert _untouched(e.u_used) and _untouched(e.v_used) and _untouched(e.sn_work), 'entry without u: something was written'
        elif e is evl:
            _check_sn(e, got, 0, what + ' (evaluation)')
        else:
            _check_sn(e, got, 1, what)
            alone = _sn_alone(L, E, e.shape)[1]
            for n in ('u', 'v', 'u_used', 'v_used', 'sigma'):
                assert _same_bits(alone[n], got[n]), '%s: %s differs from the run alone' % (what, n)
            nrb = WC.cdiv(e.rows, WC.SN_RB)
            assert _same_bits(alone['sn_work'][:nrb * e.cols + e.rows], got['sn_work'][:nrb * e.cols + e.rows])


# ---- b. gradient epilogue -------------------------------------------------------------------------------------------------------
SN, NO_SN, NO_GRAD, NO_BIAS = 'sn', 'no_sn', 'no_grad', 'no_bias'


class GradEntry:
    """one weight of an epilogue table on the device.  variant: SN (spectral norm, gradient and bias), NO_SN (u_used == NULL:
    grad == G bit-exact), NO_GRAD (grad == NULL, bias only), NO_BIAS (grad_bias == NULL)"""

    def __init__(self, case, variant=SN):
        self.c, self.variant = case, variant
        case.check_inputs()
        self.slab, self.bias_pk, self.w = case.slab.cuda(), case.bias_pk.cuda(), case.w.contiguous().cuda()
        self.u, self.v = case.u.cuda(), case.v.cuda()
        self.sigma = torch.tensor([case.sigma, float('nan')], dtype=F32).cuda()
        self.grad = Buf(case.cout * case.cols)
        self.grad_bias = Buf(case.cout)
        self.outs = [self.grad, self.grad_bias]

    def fill(self, t):
        c, var = self.c, self.variant
        t.dwpk, t.w_orig, t.sigma = self.slab.data_ptr(), self.w.data_ptr(), self.sigma.data_ptr()
        t.u_used, t.v_used = (None, None) if var == NO_SN else (self.u.data_ptr(), self.v.data_ptr())
        t.grad = None if var == NO_GRAD else self.grad.ptr()
        t.dbias_pk = self.bias_pk.data_ptr()
        t.grad_bias = None if var == NO_BIAS else self.grad_bias.ptr()
        t.Cout, t.Cin, t.KH, t.KW, t.shuffle2 = c.cout, c.cin, c.k, c.k, c.shuffle2
        for n in WC.PLAN_FIELDS:
            setattr(t, n, c.plan[n])
        t.layout = c.layout


def _check_grad(e, fast, dot_parts, what):
    """dot_parts: this entry's written slice of dot_work (one partial per tile)"""
    c, var = e.c, e.variant
    shape4 = (c.cout, c.cin, c.k, c.k)
    if var == NO_BIAS:
        assert _untouched(e.grad_bias), what + ': grad_bias == NULL but something was written'
    else:
        assert _same_bits(e.grad_bias.cpu(), c.bias), what + ': bias gradient (a copy through the channel permutation)'
    if var == NO_GRAD:
        assert _untouched(e.grad), what + ': grad == NULL but something was written'
    else:
        got = e.grad.cpu().view(shape4)
        assert bool(torch.isfinite(got).all()), what + ': a padding slot of the slab reached the gradient'
        if var == NO_SN:
            assert _same_bits(got, c.g), what + ': no spectral norm: grad must be G'
        else:
            assert c.rho >= 0.25
            assert_within(got, c.ref, c.grad_bound(fast), what + ' grad (rho %.2f)' % c.rho)
    if var in (NO_SN, NO_GRAD):
        assert bool((dot_parts == 0).all()), what + ': dot partials of an entry without a dot'
    else:       # every tile's partial against its own float64 dot: (the tile's chain) u sum|terms of the tile|
        dots, sums = c.tile_dots(fast)
        assert_within(dot_parts.reshape(-1), dots, c.dot_chain(fast)[0] * WC.U * sums, what + ' <G, W_orig> per tile')


def _run_generic(L, E, entries):
    table = (L.WeightGradDesc * len(entries))()
    for i, e in enumerate(entries):
        e.fill(table[i])
    tiles = [L.lib().sisr_weights_grad_tiles(C.byref(t)) for t in table]
    assert tiles == [e.c.n_tiles for e in entries]
    parts = max(tiles)
    tab = _table(E, table)
    work = Buf(parts * len(entries))
    run2(lambda: L.lib().sisr_weights_grad(tab.data_ptr(), len(entries), work.ptr(), parts, _st()),
         [work] + [o for e in entries for o in e.outs])
    dw = work.cpu().view(len(entries), parts)
    for i, e in enumerate(entries):
        assert bool((dw[i, tiles[i]:] == SENT).all()), 'dot_work behind the tiles of entry %d was written' % i
        _check_grad(e, False, dw[i, :tiles[i]], 'generic layout %d %s %s' % (e.c.layout, e.c.shape, e.variant))


def _run_fast(L, E, entries):
    table = (L.WeightGradDesc * len(entries))()
    for i, e in enumerate(entries):
        e.fill(table[i])
        assert e.c.layout == 1 and e.c.k == 3 and e.c.cin % 32 == 0 and not e.c.shuffle2 and e.c.plan['CoutPad'] % 32 == 0
    mco, mci = max(e.c.cout for e in entries), max(e.c.cin for e in entries)
    ty, tz = WC.cdiv(mco, 32), mci // 32
    tab = _table(E, table)
    work = Buf(len(entries) * ty * tz)
    run2(lambda: L.lib().sisr_weights_grad_fast(tab.data_ptr(), len(entries), work.ptr(), mco, mci, _st()),
         [work] + [o for e in entries for o in e.outs])
    dw = work.cpu().view(len(entries), ty, tz)
    for i, e in enumerate(entries):
        ncb, nkb = WC.cdiv(e.c.cout, 32), e.c.cin // 32
        mine = torch.zeros(ty, tz, dtype=torch.bool)
        mine[:ncb, :nkb] = True
        assert bool((dw[i][~mine] == SENT).all()), 'dot_work outside the tiles of entry %d was written' % i
        _check_grad(e, True, dw[i][mine], 'fast %s %s' % (e.c.shape, e.variant))
    return mco, mci


@pytest.mark.parametrize('shape', WC.GEN_L0, ids=_sid)
def test_grad_generic_layout0_alone(L, E, shape):
    _run_generic(L, E, [GradEntry(WC.case_of(shape, 0))])


@pytest.mark.parametrize('shape', WC.GEN_L1, ids=_sid)
def test_grad_generic_layout1_alone(L, E, shape):
    _run_generic(L, E, [GradEntry(WC.case_of(shape, 1))])


def test_grad_generic_layout1_cout3_on_the_padded_plan(L, E):
    """the generator's last conv as the engine runs it: Cout = 3 un-packed from the slab planned for 4 output channels"""
    c4 = WC.case_of((4, 64, 3, 0), 1)
    c = WC.GradCase((3, 64, 3, 0), 1, 900, plan_cout=4)
    assert c.plan == c4.plan
    _run_generic(L, E, [GradEntry(c)])


def _alone_bits(run, L, E, case):
    e = GradEntry(case)
    run(L, E, [e])
    return e.grad.cpu(), e.grad_bias.cpu()


def test_grad_generic_table_layout0(L, E):
    """every layout-0 shape in one table (`parts` = 36 from the largest; 18, 1 and 4 tiles beside it), with the three variants; the
    dot of a weight is summed in the same order whatever the grid: same bits as alone"""
    variants = [SN, NO_SN, NO_GRAD, NO_BIAS, SN, SN, SN]
    entries = [GradEntry(WC.case_of(s, 0), v) for s, v in zip(WC.GEN_L0, variants)]
    _run_generic(L, E, entries)
    for e in entries:
        if e.variant == SN:
            g, b = _alone_bits(_run_generic, L, E, e.c)
            assert _same_bits(g, e.grad.cpu()) and _same_bits(b, e.grad_bias.cpu()), e.c.shape


def test_grad_generic_table_layout1(L, E):
    variants = [SN, NO_BIAS, NO_SN, NO_GRAD, SN]
    shapes = WC.GEN_L1 + WC.FAST
    _run_generic(L, E, [GradEntry(WC.case_of(s, 1), v) for s, v in zip(shapes, variants)])


@pytest.mark.parametrize('shape', WC.FAST + WC.FAST_TABLE, ids=_sid)
def test_grad_fast_alone_and_against_generic_layout1(L, E, shape):
    """each path meets the float64 bound on its own; their mutual difference is printed"""
    c = WC.case_of(shape, 1)
    ef, eg = GradEntry(c), GradEntry(c)
    _run_fast(L, E, [ef])
    _run_generic(L, E, [eg])
    d = (ef.grad.cpu().double() - eg.grad.cpu().double()).abs().view(c.ref.shape)
    print('fast vs generic %s: max |difference| %.3e, max difference / bound %.3f'
          % (shape, float(d.max()), float((d / c.grad_bound(True)).max())))
    assert _same_bits(ef.grad_bias.cpu(), eg.grad_bias.cpu())


def test_grad_fast_table(L, E):
    """max_cout = 128 and max_cin = 128 come from different entries; the three variants ride along"""
    shapes = WC.FAST_TABLE + WC.FAST[:2]
    variants = [SN, NO_BIAS, SN, NO_SN, NO_GRAD]
    entries = [GradEntry(WC.case_of(s, 1), v) for s, v in zip(shapes, variants)]
    assert _run_fast(L, E, entries) == (128, 128)
    for e in entries:
        if e.variant == SN:
            g, b = _alone_bits(_run_fast, L, E, e.c)
            assert _same_bits(g, e.grad.cpu()) and _same_bits(b, e.grad_bias.cpu()), e.c.shape


# ---- c. packing -----------------------------------------------------------------------------------------------------------------
def _pack_layers(E):
    """(geometry, spectral norm): trunk, shuffle, 9x9 from the image, to the image, stride 2, the smallest conv_deep.hip layer"""
    G = E.ConvGeom
    return [(G(64, 64, 3), True), (G(64, 256, 3, shuffle2=True), True), (G(3, 64, 9), False), (G(64, 3, 3), False),
            (G(128, 128, 3, stride=2), True), (G(32, 64, 3), True)]


def _images(E, p):
    """[(name, the written floats of the image)] of one Prepared: a view is exactly as long as its image"""
    out = [('fwd', p.wpk_fwd)]
    if isinstance(p.wpk_dgrad, list):
        out += [('dgrad class %d' % c, v) for c, v in enumerate(p.wpk_dgrad) if v is not None]
    elif p.wpk_dgrad is not None:
        out.append(('dgrad', p.wpk_dgrad))
    out += [('sigma', p.sigma), ('inv_sigma', p.inv_sigma)]
    if p.u_used is not None:
        out += [('u_used', p.u_used), ('v_used', p.v_used)]
    return out


@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_pack_table_equals_single_entry_images(E, precision):
    """ties the multi-entry launches (grid stride from parts_for of the LARGEST weight, the max_cout / max_cin grid of the deep
    pack) to the single-entry images; evaluation mode keeps u and v fixed"""
    before = E.PRECISION
    E.set_precision(precision)
    try:
        refs = []
        for i, (gm, sn) in enumerate(_pack_layers(E)):
            w, u, v = WC.sn_inputs((gm.cout, gm.cin, gm.k), seed=40 + i)
            refs.append(FakeConv(w.reshape(gm.cout, gm.cin, gm.k, gm.k).contiguous().cuda(), None, gm,
                                 u.cuda() if sn else None, v.cuda() if sn else None))
        items = [(r, 2, 16, 16) for r in refs]
        multi, keep = E.prepare_weights(items, training=False)
        kinds = [p.kinds for p in multi]
        if precision == 'bf16':
            assert kinds[5][0] == E.Kind.DEEP and kinds[4][1] == E.Kind.DEEP_S2X4 and kinds[0][0] == E.Kind.BF16, kinds
        else:
            assert all(k == E.Kind.F32 for ks in kinds for k in ks), kinds
        n_images = 0
        for it, pm in zip(items, multi):
            single, keep1 = E.prepare_weights([it], training=False)
            a, b = _images(E, pm), _images(E, single[0])
            assert [n for n, _ in a] == [n for n, _ in b]
            for (name, x), (_, y) in zip(a, b):
                assert x.numel() > 0, (it[0].geom.cout, name)
                assert _same_bits(x.cpu(), y.cpu()), 'Cout %d Cin %d: %s differs from the single-entry table' % (
                    it[0].geom.cout, it[0].geom.cin, name)
                n_images += 1
            if it[0].u is not None:
                assert float(pm.sigma) != 1.0
        torch.cuda.synchronize()
        print('%s: %d images and scalars compared' % (precision, n_images))
    finally:
        E.set_precision(before)


def test_prepare_is_the_power_iteration_then_the_pack(L, E):
    """sisr_weights_prepare on one spectral-normalised weight with a forward image: u, v, sigma carry the bits of sisr_weights_sn
    alone, and the fp32 image [chunk][r][cp][krow = s * PS + cl] holds fl(W_orig * fl(1 / sigma)) -- one IEEE product per element,
    bit-exact -- with zeros in every padding slot"""
    shape = (64, 32, 3)
    cout, cin, k = shape
    before = E.PRECISION
    E.set_precision('fp32')
    try:
        plan = E.ConvGeom(cin, cout, k).plans(2, 16, 16)[0].plan
    finally:
        E.set_precision(before)
    CK, PS, KROWP, n_chunk, CoutPad = (getattr(plan, n) for n in WC.PLAN_FIELDS)
    assert plan.wpk_elems == n_chunk * k * CoutPad * KROWP and k * PS <= KROWP and CK <= PS and n_chunk * CK >= cin
    e, first, _ = _sn_alone(L, E, shape)
    p = SnEntry(shape)
    img = Buf(plan.wpk_elems)
    table = (L.WeightDesc * 1)()
    p.fill(table[0])
    g = table[0].img[0]
    g.dst, g.format, g.KH, g.KW, g.Sy, g.Sx = img.ptr(), L.WIMG_F32, k, k, 1, 1
    for n in WC.PLAN_FIELDS:
        setattr(g, n, getattr(plan, n))
    assert L.lib().sisr_weight_image_bytes(C.byref(g)) == 4 * plan.wpk_elems
    tab = _table(E, table)
    run2(lambda: L.lib().sisr_weights_prepare(tab.data_ptr(), 1, p.rows, p.cols, _st()), p.outs + [img])
    got = p.results()
    for n in ('u', 'v', 'u_used', 'v_used', 'sigma'):
        assert _same_bits(first[n], got[n]), 'prepare: %s differs from sisr_weights_sn' % n
    inv = np.float32(1) / np.float32(got['sigma'][0].item())
    w4 = e.w.reshape(cout, cin, k, k) * torch.tensor(inv)                       # fp32 x fp32, rounded once
    want = torch.zeros(n_chunk, k, CoutPad, KROWP)
    for ch in range(n_chunk):
        n = min(CK, cin - ch * CK)
        dst = want[ch, :, :, :k * PS].view(k, CoutPad, k, PS)                   # [r][cp][s][cl]
        dst[:, :cout, :, :n] = w4[:, ch * CK:ch * CK + n].permute(2, 0, 3, 1)
    assert _same_bits(img.cpu(), want.reshape(-1)), 'forward image of sisr_weights_prepare'
