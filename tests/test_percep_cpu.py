"""CPU: the host side of the multi-tap perceptual + Gram style loss: tap_shapes against get_size; the float64
restatement of percep_cases.py against the autograd of BasicSR's composition; the exactness claim of the exact cases, restated with
torch fp32; the derived bounds hold for torch's own fp32 composition; the entry points and the Python wrappers refuse every bad
argument before they touch a GPU; the constants of _lib are the header's."""
import ctypes as C
import os
import re

import pytest
import torch

from percep_cases import (CRITERIA, EXACT, F64, REAL, U, D_from_grams, case_id, composition, crit_grad64, exact_inputs, grad64, gram64,
                          gram_bounds, pkg, real_inputs, split, style_grad_bound, terms64, total_of)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BADARG, TOOBIG = -1, -2


def test_tap_shapes_sum_to_get_size_for_every_mask():
    ce = pkg('model_content_extractor')
    im = torch.zeros(1, 3, 32, 32)
    for mask in range(1, 32):
        net = ce.MaskedVGG(mask, width_div=4, pretrained=False)
        shapes = ce.tap_shapes(net, 32, 32)
        bits = [i for i in range(5) if mask & (1 << i)]
        assert shapes == tuple((ce.layersSize[i] // 4, 32 >> i, 32 >> i) for i in bits), mask
        assert 4 * total_of(shapes) == ce.get_size(im, mask), mask
    assert ce.tap_shapes(ce.MaskedVGG(0b00101, pretrained=False), 48, 16) == ((64, 48, 16), (256, 12, 4))
    assert ce.tap_shapes(ce.identity(), 24, 40) == ((3, 24, 40),)
    assert ce.tap_shapes(ce.vgg_4conv_1maxPool(pretrained=False), 24, 40) == ((128, 12, 20),)
    with pytest.raises(ValueError):
        ce.tap_shapes(torch.nn.ReLU(), 8, 8)


@pytest.mark.parametrize('criterion', CRITERIA)
@pytest.mark.parametrize('case', [REAL[0], REAL[3], REAL[5], REAL[6], REAL[7]], ids=case_id)
def test_restatement_is_the_composition_and_its_autograd(case, criterion):
    """terms64 against BasicSR's text, and the gradient formulas (crit_grad64 for the feature term, (2 / (C P)) D F with D from the
    Gram matrices for the style term) against its float64 autograd"""
    b, shapes, lw, relu = case
    fa, fb = (t.to(F64).requires_grad_() for t in real_inputs(b, shapes, relu))
    pw, sw = 0.75, 3.0
    percep, style = composition(fa, fb, shapes, lw, pw, sw, criterion)
    t, s = terms64(fa.detach(), fb.detach(), shapes, criterion)
    w = torch.tensor(lw, dtype=F64)
    assert abs(float(percep.detach()) - pw * float((w * t).sum())) <= 1e-13 * abs(float(percep.detach()))
    assert abs(float(style.detach()) - sw * float((w * s).sum())) <= 1e-13 * abs(float(style.detach()))
    gp, gs = 0.5, -1.5
    da, db = torch.autograd.grad(gp * percep + gs * style, (fa, fb))
    fa, fb = fa.detach(), fb.detach()
    ga, gb = gram64(fa, shapes), gram64(fb, shapes)
    want_a, want_b = [], []
    for l, (xa, xb) in enumerate(zip(split(fa, shapes), split(fb, shapes))):
        d = crit_grad64(ga[l] - gb[l], criterion)
        feat = gp * pw * lw[l] * crit_grad64(xa - xb, criterion)
        want_a.append((feat + gs * sw * lw[l] * grad64(xa, d)).reshape(b, -1))
        want_b.append((-feat - gs * sw * lw[l] * grad64(xb, d)).reshape(b, -1))
    ea = float((torch.cat(want_a, 1) - da).abs().max() / da.abs().max())
    eb = float((torch.cat(want_b, 1) - db).abs().max() / db.abs().max())
    print('%s %s: formula - autograd, of the largest gradient: %.3e (dfa), %.3e (dfb)' % (case_id(case), criterion, ea, eb))
    assert ea <= 1e-12 and eb <= 1e-12


@pytest.mark.parametrize('case', EXACT, ids=case_id)
def test_exact_cases_are_exact_in_fp32(case):
    """torch's own fp32 composition of the Gram matrices reproduces float64 bit for bit, and the cases contain exact ties"""
    b, shapes, _ = case
    fa, fb = exact_inputs(b, shapes)
    ties = 0.0
    for x in (fa, fb):
        for f, g in zip(split(x, shapes), gram64(x, shapes)):
            g32 = f.bmm(f.transpose(1, 2)) / (f.shape[1] * f.shape[2])
            assert torch.equal(g32.to(F64), g)
    for a, c in zip(gram64(fa, shapes), gram64(fb, shapes)):
        ties = max(ties, float((a == c).to(F64).mean()))
    print('%s: largest share of ties G_a == G_b over the taps %.4f' % (case_id(case), ties))
    assert ties > 0


@pytest.mark.parametrize('case', REAL, ids=case_id)
def test_torch_fp32_composition_is_inside_the_derived_bounds(case):
    """the bounds the kernels are held to leave room for a correct fp32 evaluation: torch's own stays inside them"""
    b, shapes, lw, relu = case
    fa, fb = real_inputs(b, shapes, relu)
    worst_g, worst_d = 0.0, 0.0
    for x in (fa, fb):
        for f, g, e in zip(split(x, shapes), gram64(x, shapes), gram_bounds(x, shapes)):
            g32 = f.bmm(f.transpose(1, 2)) / (f.shape[1] * f.shape[2])
            worst_g = max(worst_g, float(((g32.to(F64) - g).abs() / e.clamp_min(1e-300)).max()))
    for xa, xb in zip(split(fa, shapes), split(fb, shapes)):
        c, p = xa.shape[1:]
        ga, gb = (x.bmm(x.transpose(1, 2)) / (c * p) for x in (xa, xb))
        d = D_from_grams(ga, gb, 'l2')
        got = (2.0 / (c * p)) * torch.bmm(d.to(torch.float32), xa)
        worst_d = max(worst_d, float(((got.to(F64) - grad64(xa, d)).abs() / style_grad_bound(xa, d, 1.0).clamp_min(1e-300)).max()))
    print('%s: torch fp32 uses %.3f of the Gram bound, %.3f of the gradient bound' % (case_id(case), worst_g, worst_d))
    assert worst_g <= 1.0 and worst_d <= 1.0


def test_lib_constants_are_the_headers():
    L = pkg('_lib')
    hdr = open(os.path.join(ROOT, 'include', 'sisr_hip.h')).read()
    defs = dict(re.findall(r'#define (SISR_PERCEP_[A-Z0-9_]+) (\d+)', hdr))
    assert {k: int(v) for k, v in defs.items()} == {'SISR_PERCEP_MAX_TAPS': L.PERCEP_MAX_TAPS, 'SISR_PERCEP_L1': L.PERCEP_L1,
                                                    'SISR_PERCEP_L2': L.PERCEP_L2, 'SISR_PERCEP_FRO': L.PERCEP_FRO}
    assert L.PERCEP_MAX_TAPS == 8 and pkg('losses').PERCEP_CRITERIA == {'l1': L.PERCEP_L1, 'l2': L.PERCEP_L2, 'fro': L.PERCEP_FRO}


def _shapes(*taps):
    return (C.c_int32 * (3 * len(taps)))(*[v for s in taps for v in s])


def test_every_bad_argument_is_refused_without_a_gpu():
    lib = pkg('_lib').lib()
    buf = (C.c_double * 8)()
    # non-null, 16-byte aligned pointers 16 MiB apart: every call here is refused, refused calls never read them, and nothing reaches
    # a launch
    base = (C.cast(buf, C.c_void_p).value + 15) & ~15
    p, q, r, s, t, u, v = (C.c_void_p(base + (i << 24)) for i in range(1, 8))
    one, three = _shapes((4, 2, 2)), _shapes((4, 2, 2), (8, 1, 1), (2, 3, 1))
    nine = _shapes(*[(1, 1, 1)] * 9)
    w = (C.c_float * 9)(*[1.0] * 9)
    # the size query: doubles for the two reductions, then the partials of both inputs
    both = lib.sisr_percep_ws_bytes(2, 3, three, 1, 1)
    feat, sty = lib.sisr_percep_ws_bytes(2, 3, three, 1, 0), lib.sisr_percep_ws_bytes(2, 3, three, 0, 1)
    assert feat > 0 and feat % 16 == 0 and sty >= 4 * 2 * 2 * (16 + 64 + 4) and both == feat + sty
    assert lib.sisr_percep_ws_bytes(2, 3, three, 0, 0) == 0
    for bad in ((0, 1, one), (-1, 1, one), (2, 0, one), (2, 9, nine), (2, 1, None), (2, 1, _shapes((0, 2, 2))), (2, 1, _shapes((4, -1, 2))),
                (2, 1, _shapes((4, 2, 0)))):
        assert lib.sisr_percep_ws_bytes(*bad, 1, 1) == BADARG, bad[:2]
    assert lib.sisr_percep_ws_bytes(1, 1, _shapes((1 << 16, 1 << 10, 1 << 10)), 1, 1) == TOOBIG
    good = dict(f=p, B=2, total=16, n=1, shapes=one, ws=q, gram=r, stream=None)
    for bad in (dict(f=None), dict(ws=None), dict(gram=None), dict(ws=C.c_void_p(q.value + 8)), dict(B=0), dict(n=0), dict(n=9, shapes=nine, total=9),
                dict(total=15), dict(total=0), dict(shapes=None), dict(shapes=_shapes((4, 0, 4)))):
        assert lib.sisr_percep_gram(*dict(good, **bad).values()) == BADARG, bad
    good = dict(fa=p, fb=q, B=2, total=30, n=3, shapes=three, lw=w, pw=1.0, sw=1.0, crit=0, ws=r, tp=s, ts=t, percep=u, style=v, dmat=None,
                stream=None)
    for bad in (dict(fa=None), dict(fb=None), dict(ws=None), dict(lw=None), dict(shapes=None), dict(ws=C.c_void_p(r.value + 4)), dict(B=0),
                dict(B=-3), dict(n=0), dict(n=-1), dict(n=9, shapes=nine, total=9), dict(total=29), dict(total=31), dict(crit=3), dict(crit=-1),
                dict(shapes=_shapes((4, 2, 2), (8, 0, 1), (2, 3, 1))), dict(percep=None), dict(style=None), dict(pw=0.0, sw=0.0)):
        assert lib.sisr_percep_fwd(*dict(good, **bad).values()) == BADARG, bad
    good = dict(fa=p, fb=q, dmat=r, tp=s, ts=t, gp=u, gs=v, B=2, total=30, n=3, shapes=three, lw=w, pw=1.0, sw=1.0, crit=0, dfa=p, dfb=q,
                stream=None)
    for bad in (dict(fa=None), dict(fb=None), dict(dmat=None), dict(gp=None), dict(gs=None), dict(dfa=None, dfb=None), dict(lw=None),
                dict(shapes=None), dict(B=0), dict(n=0), dict(n=9, shapes=nine, total=9), dict(total=29), dict(crit=5), dict(crit=2, tp=None),
                dict(crit=2, ts=None), dict(pw=0.0, sw=0.0)):
        assert lib.sisr_percep_bwd(*dict(good, **bad).values()) == BADARG, bad


def test_python_wrappers_validate_and_refuse_cpu_tensors():
    Lm, top = pkg('losses'), pkg()
    assert top.perceptual_loss is Lm.perceptual_loss and top.gram_matrix is Lm.gram_matrix and top.PerceptualLoss is Lm.PerceptualLoss
    shapes = ((4, 2, 2), (2, 3, 1))
    x = torch.zeros(2, 22)
    with pytest.raises(RuntimeError):
        Lm.perceptual_loss(x, x, shapes)                            # CPU tensors: no fallback
    with pytest.raises(RuntimeError):
        Lm.perceptual_loss(x, x, shapes, style_weight=1.0, criterion='fro')
    with pytest.raises(RuntimeError):
        Lm.gram_matrix(x, shapes)
    for bad in (((4, 2, 2),), ((4, 2, 2), (2, 3, 2)), ((1, 1, 1),) * 9, ((4, 2, 2), (2, 3, 0), (1, 1, 6)), ((4, 2), (2, 3, 1)), (), 7,
                ((4, 2, 2), (2, -3, -1))):
        with pytest.raises(ValueError):
            Lm.perceptual_loss(x, x, bad)
        with pytest.raises(ValueError):
            Lm.gram_matrix(x, bad)
    nine = torch.zeros(2, 9)
    with pytest.raises(ValueError, match='1 .. 8 taps'):
        Lm.perceptual_loss(nine, nine, ((1, 1, 1),) * 9)
    for bad in ('L1', 'mse', None, 1):
        with pytest.raises(ValueError, match='criterion'):
            Lm.perceptual_loss(x, x, shapes, criterion=bad)
    for bad in (x.double(), x.half(), x.to(torch.bfloat16), None, torch.zeros(2, 23), torch.zeros(3, 22), torch.zeros(0, 22), torch.zeros(2, 2, 11)):
        with pytest.raises(ValueError):
            Lm.perceptual_loss(bad, x, shapes)
        with pytest.raises(ValueError):
            Lm.perceptual_loss(x, bad, shapes)
    for bad in (x.double(), None, torch.zeros(2, 23), torch.zeros(2, 2, 11)):
        with pytest.raises(ValueError):
            Lm.gram_matrix(bad, shapes)
    for bad in (dict(layer_weights=(1.0,)), dict(layer_weights=(1.0, float('nan'))), dict(perceptual_weight=float('inf')),
                dict(style_weight=float('nan'))):
        with pytest.raises(ValueError):
            Lm.perceptual_loss(x, x, shapes, **bad)
    with pytest.raises(ValueError, match='criterion'):
        Lm.PerceptualLoss(pkg('model_content_extractor').identity(), criterion='huber')
    with pytest.raises(RuntimeError):
        Lm.PerceptualLoss(pkg('model_content_extractor').identity())(torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, 4, 4))


def test_one_rounding_is_what_the_exact_tests_mean():
    """u = 2^-24 is the largest relative distance of a float64 value from its fp32 rounding"""
    v = torch.tensor([1.0 + 2.0 ** -24 + 2.0 ** -40, 3.0 - 2.0 ** -23], dtype=F64)
    assert bool(((v.to(torch.float32).to(F64) - v).abs() <= U * v.abs()).all()) and U == 2.0 ** -24
