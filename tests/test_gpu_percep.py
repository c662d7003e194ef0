"""GPU: the multi-tap perceptual + Gram style loss (csrc/percep.hip, losses.perceptual_loss / gram_matrix / PerceptualLoss; DESIGN.md
section 29) against the float64 restatement of percep_cases.py, through the C entry points (guards around every output and the
workspace, two launches with identical bits) and through the Python surface.

Bounds (percep_cases.py), derived and not measured.  EXACT cases (power-of-two sizes and weights, integer features): the Gram
matrices EQUAL float64 and are bit-symmetric, 'l1' terms and gradients are within one fp32 rounding of float64, 'l2' / 'fro' terms
within four.  REAL cases: |G - G64| <= (P + 2) u (|F| |F|^T) / (C P) element by element; the terms within the propagated sum of those
plus four roundings; the style gradient against (2 / (C P)) D F in float64 on the DEVICE's own D (from gram_matrix on the same inputs,
whose bits are the loss's internal ones) within (C + 4) u c (|D| |F|), element by element, nothing left out.  One end-to-end
comparison with the float64 autograd of BasicSR's composition: 'l2', 1e-3 of the sample's largest gradient."""
import ctypes as C

import pytest
import torch

from gpu_helpers import Buf, run2
from percep_cases import (CRITERIA, EXACT, EXACT_MULTI, F64, REAL, REAL_MULTI, U, D_from_grams, case_id, composition, crit_grad64,
                          exact_inputs, grad64, gram64, gram_bounds, pkg, real_inputs, split, style_grad_bound, style_term_bounds, terms64,
                          total_of)

pytestmark = pytest.mark.gpu
CODES = {'l1': 0, 'l2': 1, 'fro': 2}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _inputs(case):
    if len(case) == 3:
        return exact_inputs(case[0], case[1])
    return real_inputs(case[0], case[1], case[3])


def _within(got, ref, bound, what):
    err = (got.detach().cpu().to(F64) - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print('%s: max err %.3e, max err / bound %.3f' % (what, float(err.max()), ratio))
    assert bool((err <= bound).all()), (what, float(err.max()), ratio)


def _shape_array(shapes):
    return (C.c_int32 * (3 * len(shapes)))(*[v for s in shapes for v in s])


def _run(case, criterion, pw, sw, g=(1.0, 1.0), need=(True, True)):
    """-> (percep, style, terms_p, terms_s, dfa, dfb) through losses.perceptual_loss and autograd"""
    Lm = pkg('losses')
    fa, fb = (t.cuda().requires_grad_(n) for t, n in zip(_inputs(case), need))
    percep, style, tp, ts = Lm.perceptual_loss(fa, fb, case[1], case[2], pw, sw, criterion, return_terms=True)
    loss = sum(gi * t for gi, t in zip(g, (percep, style)) if t is not None)
    loss.backward()
    return percep, style, tp, ts, fa.grad, fb.grad


# ---- through the C entry points ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', [EXACT_MULTI, REAL_MULTI, REAL[7], REAL[1]], ids=case_id)
def test_entry_points_keep_their_guards_and_their_bits(case):
    Lm, lib = pkg('losses'), pkg('_lib').lib()
    b, shapes, lw = case[:3]
    fa, fb = (t.cuda() for t in _inputs(case))
    n, total, arr = len(shapes), total_of(shapes), _shape_array(shapes)
    w = (C.c_float * n)(*lw)
    nd = sum(b * c * c for c, _, _ in shapes)
    ws = Buf(lib.sisr_percep_ws_bytes(b, n, arr, 1, 1) // 4)
    tp, ts, percep, style, dmat, gram = Buf(n), Buf(n), Buf(1), Buf(1), Buf(nd), Buf(nd)
    run2(lambda: lib.sisr_percep_gram(fa.data_ptr(), b, total, n, arr, ws.ptr(), gram.ptr(), _stream()), [gram, ws])
    want = torch.cat([g.reshape(-1) for g in Lm.gram_matrix(fa, shapes)])
    assert torch.equal(gram.body, want)
    for criterion in CRITERIA:
        call = lambda: lib.sisr_percep_fwd(fa.data_ptr(), fb.data_ptr(), b, total, n, arr, w, 0.75, 2.0, CODES[criterion], ws.ptr(),   # noqa: E731
                                           tp.ptr(), ts.ptr(), percep.ptr(), style.ptr(), dmat.ptr(), _stream())
        run2(call, [tp, ts, percep, style, dmat, ws])
        a, c = fa.clone().requires_grad_(), fb.clone().requires_grad_()
        p2, s2, tp2, ts2 = Lm.perceptual_loss(a, c, shapes, lw, 0.75, 2.0, criterion, return_terms=True)
        assert torch.equal(percep.body[0], p2) and torch.equal(style.body[0], s2)
        assert torch.equal(tp.body, tp2) and torch.equal(ts.body, ts2)
        (0.5 * p2 + 2.0 * s2).backward()
        gp, gs = torch.tensor([0.5], device='cuda'), torch.tensor([2.0], device='cuda')
        dfa, dfb = Buf(b * total), Buf(b * total)
        for pa, pb in ((True, True), (True, False), (False, True)):
            call = lambda: lib.sisr_percep_bwd(fa.data_ptr(), fb.data_ptr(), dmat.ptr(), tp.ptr(), ts.ptr(), gp.data_ptr(), gs.data_ptr(),   # noqa: E731
                                               b, total, n, arr, w, 0.75, 2.0, CODES[criterion], dfa.ptr() if pa else None,
                                               dfb.ptr() if pb else None, _stream())
            run2(call, [dfa, dfb])
            for on, buf, ref in ((pa, dfa, a.grad), (pb, dfb, c.grad)):
                if on:
                    assert torch.equal(buf.body.view(b, total), ref)
                else:
                    assert bool((buf.body == buf.fill).all())          # the gradient that was not asked for is not written


@pytest.mark.parametrize('which', ['style_off', 'perceptual_off'])
def test_a_term_with_weight_zero_is_none_and_writes_nothing(which):
    Lm, lib = pkg('losses'), pkg('_lib').lib()
    b, shapes, lw = EXACT_MULTI
    fa, fb = (t.cuda() for t in exact_inputs(b, shapes))
    pw, sw = (1.0, 0.0) if which == 'style_off' else (0.0, 1.0)
    percep, style, tp, ts = Lm.perceptual_loss(fa, fb, shapes, lw, pw, sw, return_terms=True)
    off = (style, ts) if which == 'style_off' else (percep, tp)
    on = (percep, tp) if which == 'style_off' else (style, ts)
    assert off == (None, None) and on[0].shape == () and on[1].shape == (len(shapes),)
    assert Lm.perceptual_loss(fa, fb, shapes, lw, 0.0, 0.0) == (None, None)
    n, total, arr = len(shapes), total_of(shapes), _shape_array(shapes)
    w = (C.c_float * n)(*lw)
    feat_bytes = lib.sisr_percep_ws_bytes(b, n, arr, 1, 0)
    ws = Buf(lib.sisr_percep_ws_bytes(b, n, arr, 1, 1) // 4)
    tpb, tsb, pb, sb, dmat = Buf(n), Buf(n), Buf(1), Buf(1), Buf(sum(b * c * c for c, _, _ in shapes))
    run2(lambda: lib.sisr_percep_fwd(fa.data_ptr(), fb.data_ptr(), b, total, n, arr, w, pw, sw, 0, ws.ptr(), tpb.ptr(), tsb.ptr(), pb.ptr(),
                                     sb.ptr(), dmat.ptr(), _stream()), [tpb, tsb, pb, sb, dmat, ws])
    untouched = lambda t: bool((t == ws.fill).all())              # noqa: E731
    if which == 'style_off':
        # the style term's part of the workspace (behind the feature pass's partials), D and its outputs keep their fill
        assert untouched(ws.body[feat_bytes // 4:]) and untouched(dmat.body) and untouched(tsb.body) and untouched(sb.body)
        assert torch.equal(pb.body[0], percep) and torch.equal(tpb.body, tp)
    else:
        # a style-only call lays its workspace out without the feature part: nothing of the perceptual term is written anywhere
        assert untouched(tpb.body) and untouched(pb.body)
        assert torch.equal(sb.body[0], style) and torch.equal(tsb.body, ts)
        assert untouched(ws.body[lib.sisr_percep_ws_bytes(b, n, arr, 0, 1) // 4:])


# ---- Gram matrices --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', EXACT, ids=case_id)
def test_gram_exact_cases_equal_float64(case):
    Lm = pkg('losses')
    b, shapes, _ = case
    for x in exact_inputs(b, shapes):
        got = Lm.gram_matrix(x.cuda(), shapes)
        for g, ref in zip(got, gram64(x, shapes)):
            assert g.shape == ref.shape and g.dtype == torch.float32 and not g.requires_grad
            assert torch.equal(g.cpu().to(F64), ref)
            assert torch.equal(g, g.transpose(1, 2))


@pytest.mark.parametrize('case', REAL, ids=case_id)
def test_gram_real_cases_within_the_chain_bound(case):
    Lm = pkg('losses')
    b, shapes = case[:2]
    for k, x in enumerate(_inputs(case)):
        got = Lm.gram_matrix(x.cuda(), shapes)
        for l, (g, ref, bound) in enumerate(zip(got, gram64(x, shapes), gram_bounds(x, shapes))):
            _within(g, ref, bound, 'gram %s input %d tap %d' % (case_id(case), k, l))
            assert torch.equal(g, g.transpose(1, 2))                  # bit-symmetric


# ---- terms ----------------------------------------------------------------------------------------------------------------------------
def _exact_criteria(case):
    return CRITERIA if case is EXACT_MULTI else ('l1',)


@pytest.mark.parametrize('case', EXACT, ids=case_id)
def test_terms_exact_cases(case):
    b, shapes, lw = case
    fa, fb = exact_inputs(b, shapes)
    for criterion in _exact_criteria(case):
        percep, style, tp, ts = _run(case, criterion, 0.5, 4.0)[:4]
        t64, s64 = terms64(fa, fb, shapes, criterion)
        k = 1 if criterion == 'l1' else 4
        w = torch.tensor(lw, dtype=F64)
        _within(tp, t64, k * U * t64, 'T %s %s' % (case_id(case), criterion))
        _within(ts, s64, k * U * s64, 'S %s %s' % (case_id(case), criterion))
        _within(percep, 0.5 * (w * t64).sum(), k * U * 0.5 * (w * t64).sum(), 'perceptual %s %s' % (case_id(case), criterion))
        _within(style, 4.0 * (w * s64).sum(), k * U * 4.0 * (w * s64).sum(), 'style %s %s' % (case_id(case), criterion))


def _real_criteria(case):
    return CRITERIA if case[1] == REAL_MULTI[1] else ('l1',)


@pytest.mark.parametrize('case', REAL, ids=case_id)
def test_terms_real_cases(case):
    b, shapes, lw = case[:3]
    fa, fb = _inputs(case)
    for criterion in _real_criteria(case):
        percep, style, tp, ts = _run(case, criterion, 0.75, 3.0)[:4]
        t64, s64 = terms64(fa, fb, shapes, criterion)
        sb = style_term_bounds(fa, fb, shapes, criterion)
        w = torch.tensor(lw, dtype=F64)
        _within(tp, t64, 4 * U * t64, 'T %s %s' % (case_id(case), criterion))
        _within(ts, s64, sb, 'S %s %s' % (case_id(case), criterion))
        _within(percep, 0.75 * (w * t64).sum(), 0.75 * (w * 4 * U * t64).sum() + U * 0.75 * (w * t64).sum(), 'perceptual ' + case_id(case))
        _within(style, 3.0 * (w * s64).sum(), 3.0 * (w * sb).sum() + U * 3.0 * (w * s64).sum(), 'style ' + case_id(case))


# ---- gradients ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pw', [0.0, 2.0], ids=['style_alone', 'style_plus_feature'])
@pytest.mark.parametrize('case', EXACT, ids=case_id)
def test_l1_gradients_exact_cases_within_one_rounding(case, pw):
    Lm = pkg('losses')
    b, shapes, lw = case
    fa, fb = exact_inputs(b, shapes)
    sw, g = 0.5, (0.25, 2.0)                                       # powers of two: the loss weights and the upstream gradients
    dfa, dfb = _run(case, 'l1', pw, sw, g)[4:]
    ga, gb = Lm.gram_matrix(fa.cuda(), shapes), Lm.gram_matrix(fb.cuda(), shapes)
    want_a, want_b = [], []
    for l, (xa, xb) in enumerate(zip(split(fa, shapes), split(fb, shapes))):
        d = D_from_grams(ga[l].cpu(), gb[l].cpu(), 'l1')
        feat = g[0] * pw * lw[l] * crit_grad64(xa - xb, 'l1')
        want_a.append((feat + g[1] * sw * lw[l] * grad64(xa, d)).reshape(b, -1))
        want_b.append((-feat - g[1] * sw * lw[l] * grad64(xb, d)).reshape(b, -1))
    want_a, want_b = torch.cat(want_a, 1), torch.cat(want_b, 1)
    assert float(want_a.abs().max()) > 0
    _within(dfa, want_a, U * want_a.abs(), 'dfa %s' % case_id(case))
    _within(dfb, want_b, U * want_b.abs(), 'dfb %s' % case_id(case))


@pytest.mark.parametrize('case', REAL, ids=case_id)
def test_style_gradients_real_cases_on_the_devices_own_D(case):
    Lm = pkg('losses')
    b, shapes, lw = case[:3]
    fa, fb = _inputs(case)
    sw, g = 3.0, (1.0, 0.625)
    ga, gb = Lm.gram_matrix(fa.cuda(), shapes), Lm.gram_matrix(fb.cuda(), shapes)
    for criterion in _real_criteria(case):
        dfa, dfb = _run(case, criterion, 0.0, sw, g)[4:]
        for l, (xa, xb) in enumerate(zip(split(fa, shapes), split(fb, shapes))):
            d = D_from_grams(ga[l].cpu(), gb[l].cpu(), criterion)
            coeff = g[1] * sw * lw[l]
            for name, got, x, sign in (('dfa', dfa, xa, 1.0), ('dfb', dfb, xb, -1.0)):
                _within(split(got, shapes)[l], sign * coeff * grad64(x, d), style_grad_bound(x, d, coeff),
                        '%s %s %s tap %d' % (name, case_id(case), criterion, l))


@pytest.mark.parametrize('criterion', CRITERIA)
def test_feature_term_alone_and_one_sided_gradients(criterion):
    """only the feature term: dfb == -dfa bit for bit, each within four roundings of the float64 formula; a call that needs one
    gradient computes that one, the same bits"""
    case = REAL_MULTI
    b, shapes, lw = case[:3]
    fa, fb = _inputs(case)
    percep, style, _, _, dfa, dfb = _run(case, criterion, 0.75, 0.0, (0.625, 1.0))
    assert style is None and torch.equal(dfb, -dfa)
    want = torch.cat([(0.625 * 0.75 * lw[l] * crit_grad64(xa - xb, criterion)).reshape(b, -1)
                      for l, (xa, xb) in enumerate(zip(split(fa, shapes), split(fb, shapes)))], 1)
    _within(dfa, want, 4 * U * want.abs(), 'feature-only dfa %s' % criterion)
    both = _run(case, criterion, 0.75, 3.0, (0.625, 0.375))
    only_a = _run(case, criterion, 0.75, 3.0, (0.625, 0.375), need=(True, False))
    only_b = _run(case, criterion, 0.75, 3.0, (0.625, 0.375), need=(False, True))
    assert only_a[5] is None and only_b[4] is None
    assert torch.equal(only_a[4], both[4]) and torch.equal(only_b[5], both[5])
    assert all(torch.equal(x, y) for x, y in zip(only_a[:4], both[:4]))


@pytest.mark.parametrize('case', [c for c in REAL if max(s[1] * s[2] for s in c[1]) <= 64], ids=case_id)
def test_end_to_end_against_float64_autograd(case):
    b, shapes, lw = case[:3]
    fa, fb = _inputs(case)
    percep, style, _, _, dfa, dfb = _run(case, 'l2', 0.75, 3.0, (0.625, 0.375))
    a64, b64 = fa.to(F64).requires_grad_(), fb.to(F64).requires_grad_()
    p64, s64 = composition(a64, b64, shapes, lw, 0.75, 3.0, 'l2')
    da, db = torch.autograd.grad(0.625 * p64 + 0.375 * s64, (a64, b64))
    for name, got, ref in (('dfa', dfa, da), ('dfb', dfb, db)):
        rel = float(((got.cpu().to(F64) - ref).abs().amax(dim=1) / ref.abs().amax(dim=1)).max())
        print('%s %s: of the largest gradient of the sample %.3e (bound 1e-3)' % (name, case_id(case), rel))
        assert rel <= 1e-3
    assert abs(float(percep.detach()) - float(p64.detach())) <= 1e-3 * abs(float(p64.detach()))
    assert abs(float(style.detach()) - float(s64.detach())) <= 1e-3 * abs(float(s64.detach()))


# ---- properties ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('criterion', CRITERIA)
def test_equal_inputs_give_exact_zeros(criterion):
    Lm = pkg('losses')
    b, shapes, lw = REAL_MULTI[:3]
    x = _inputs(REAL_MULTI)[0].cuda()
    a, c = x.clone().requires_grad_(), x.clone().requires_grad_()
    percep, style, tp, ts = Lm.perceptual_loss(a, c, shapes, lw, 0.75, 3.0, criterion, return_terms=True)
    (percep + style).backward()
    for t in (percep, style, tp, ts, a.grad, c.grad):
        assert torch.equal(t, torch.zeros_like(t)), 'not exactly zero (or a NaN)'


def test_one_nan_feature_gives_nan_terms_without_a_fault():
    Lm = pkg('losses')
    b, shapes, lw = REAL_MULTI[:3]
    fa, fb = (t.cuda() for t in _inputs(REAL_MULTI))
    bad = fa.clone()
    bad[1, 45 + 7] = float('nan')                                  # inside the second tap
    for criterion in CRITERIA:
        a = bad.clone().requires_grad_()
        percep, style, tp, ts = Lm.perceptual_loss(a, fb, shapes, lw, 1.0, 1.0, criterion, return_terms=True)
        (percep + style).backward()
        torch.cuda.synchronize()
        clean = Lm.perceptual_loss(fa, fb, shapes, lw, 1.0, 1.0, criterion, return_terms=True)
        nan = torch.tensor([False, True, False], device='cuda')
        assert torch.equal(torch.isnan(tp), nan) and torch.equal(torch.isnan(ts), nan)
        assert torch.equal(tp[~nan], clean[2][~nan]) and torch.equal(ts[~nan], clean[3][~nan])
        assert bool(torch.isnan(percep)) and bool(torch.isnan(style))


def test_perceptual_loss_module_through_the_extractor():
    """PerceptualLoss around a MaskedVGG: the image gradient against the same extractor followed by BasicSR's composition in fp32
    torch ops -- the plumbing through VGGFunction.backward, input_norm and range_norm"""
    Lm, ce = pkg('losses'), pkg('model_content_extractor')
    net = ce.MaskedVGG(0b00111, width_div=4, pretrained=False).cuda()
    lw = (0.5, 1.0, 2.0)
    mod = Lm.PerceptualLoss(net, lw, 1.0, 2.0, 'l1', input_norm=True, range_norm=True).cuda()
    gen = torch.Generator().manual_seed(5)
    x, gt = (2 * torch.rand((2, 3, 16, 16), generator=gen) - 1 for _ in range(2))
    xd = x.cuda().requires_grad_()
    percep, style = mod(xd, gt.cuda())
    (percep + style).backward()
    shapes = ce.tap_shapes(net, 16, 16)
    assert shapes == ((16, 16, 16), (32, 8, 8), (64, 4, 4))
    xr = x.cuda().requires_grad_()
    mean, std = mod.mean.cuda(), mod.std.cuda()
    with torch.no_grad():
        fg = net(((gt.cuda() + 1) / 2 - mean) / std)
    p2, s2 = composition(net(((xr + 1) / 2 - mean) / std), fg, shapes, lw, 1.0, 2.0, 'l1')
    (p2 + s2).backward()
    percep, style, p2, s2 = (t.detach() for t in (percep, style, p2, s2))
    rel = float((xd.grad - xr.grad).abs().max() / xr.grad.abs().max())
    print('image gradient: %.3e of its largest element (bound 1e-3); losses %g %g vs %g %g' % (rel, float(percep), float(style), float(p2),
                                                                                              float(s2)))
    assert float(xr.grad.abs().max()) > 0 and rel <= 1e-3
    assert abs(float(percep) - float(p2)) <= 1e-3 * abs(float(p2)) and abs(float(style) - float(s2)) <= 1e-3 * abs(float(s2))


def test_forward_and_backward_are_capturable():
    """torch.cuda.graph captures perceptual_loss forward + backward; three replays on new contents of the static inputs are bit-equal
    to eager calls on those contents"""
    Lm = pkg('losses')
    b, shapes, lw = EXACT_MULTI
    s_a, s_b = (torch.zeros(b, total_of(shapes), device='cuda') for _ in range(2))

    def run(fa, fb):
        a, c = fa.detach().requires_grad_(), fb.detach().requires_grad_()
        percep, style, tp, ts = Lm.perceptual_loss(a, c, shapes, lw, 0.5, 2.0, 'l1', return_terms=True)
        da, dc = torch.autograd.grad(percep + style, (a, c))
        return percep.detach(), style.detach(), tp, ts, da, dc
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            run(s_a, s_b)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run(s_a, s_b)
    for rep in range(3):
        fa, fb = (t.cuda() for t in exact_inputs(b, shapes, seed=10 + rep))
        s_a.copy_(fa)
        s_b.copy_(fb)
        graph.replay()
        torch.cuda.synchronize()
        eager = run(fa, fb)
        assert all(torch.equal(x, y) for x, y in zip(out, eager)), rep
        assert float(out[0]) > 0 and float(out[1]) > 0
