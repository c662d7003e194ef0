"""GPU: the contextual loss (csrc/contextual.hip, losses.contextual_loss / contextual_similarity / ContextualLoss)
against the float64 restatement of contextual_cases.py.  u = 2^-24; every bound is derived there from the arithmetic, none from a
kernel's output:
  S element by element against float64 from the raw inputs: (C + 6) u sum_c |x^_ic| |y^_jc| plus the normalisation's roundings
  (sim_bound); everything behind S -- m, j*, Z, c, i*, CX[n], the terms, the scalar -- against the restatement evaluated on the DEVICE's
  own S with the fp32 1 - S repeated on the host, so that no near-tie can fall differently and nothing is left out (row_bounds,
  term_bound); the gradient against the float64 formulas on the device's own S and tables (grad_bound); one end-to-end comparison with
  the float64 autograd of the composition from the raw inputs, held to 4 x the distance of the fp32 torch composition on the same
  inputs, measured in the same test (DESIGN.md section 31 has the figures of an MI355X)."""
import math

import pytest
import torch

import contextual_cases as cc
from contextual_cases import BAND, CASES, F64, KINDS, SMALL, U, case_id, composition, pkg, split, total_of

pytestmark = pytest.mark.gpu
G, WEIGHT = 0.7, 1.5                # an upstream gradient and a loss weight that are not 1
BOTH = [(c, k) for c in CASES for k in KINDS]


def _id(ck):
    return case_id(ck[0]) + '-' + ck[1]


def _inputs(case, kind):
    return cc.inputs(case[0], case[1], case[3], kind)


def _within(got, ref, bound, what):
    err = (got.detach().cpu().to(F64) - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print('%s: max err %.3e, max err / bound %.3f' % (what, float(err.max()), ratio))
    assert bool((err <= bound).all()), (what, float(err.max()), ratio)


@pytest.mark.parametrize('ck', BOTH, ids=_id)
def test_similarity_against_float64(ck):
    case, kind = ck
    fa, fb = _inputs(case, kind)
    got = pkg('losses').contextual_similarity(fa.cuda(), fb.cuda(), case[1])
    assert len(got) == len(case[1])
    for l, (s, (ref, _), bound) in enumerate(zip(got, cc.sim64(fa, fb, case[1]), cc.sim_bound(fa, fb, case[1]))):
        assert s.shape == ref.shape and s.dtype == torch.float32 and not s.requires_grad
        _within(s, ref, bound, 'S of tap %d' % l)


@pytest.mark.parametrize('ck', BOTH, ids=_id)
def test_forward_and_gradient_against_float64_on_the_devices_own_similarity(ck):
    case, kind = ck
    Lm = pkg('losses')
    b, shapes, lw, _ = case
    fa, fb = _inputs(case, kind)
    a, c = fa.cuda().requires_grad_(), fb.cuda()
    sims = [s.cpu() for s in Lm.contextual_similarity(a, c, shapes)]
    tabs = Lm._contextual_tables(a, c, shapes, BAND)
    loss, terms, cx = Lm.contextual_loss(a, c, shapes, lw, BAND, WEIGHT, return_terms=True)
    (G * loss).backward()
    assert loss.dim() == 0 and loss.dtype == torch.float32 and terms.shape == (len(shapes),) and cx.shape == (len(shapes), b)
    assert not terms.requires_grad and not cx.requires_grad
    want_loss, want_terms, want_cx, taps = cc.forward64(fa, fb, shapes, lw, BAND, WEIGHT, sims=sims)
    e_loss, grads = 0.0, split(a.grad.cpu(), shapes)
    for l, (r, t, wl) in enumerate(zip(taps, tabs, lw)):
        t = {k: v.cpu() for k, v in t.items()}
        eb = cc.row_bounds(r, BAND)
        # the row pass: the fp32 min of the device's own d and its lowest index are reproduced exactly
        assert torch.equal(t['m'].to(F64), r['m']) and torch.equal(t['jstar'].long(), r['jstar']), 'm / j* of tap %d' % l
        _within(t['Z'], r['Z'], eb['eZ'], 'Z of tap %d' % l)
        _within(t['c'], r['c'], eb['ec'], 'c of tap %d' % l)
        # i*: an index whose float64 CX is the column's largest up to the two errors
        at = r['CX'].gather(1, t['istar'].long().unsqueeze(1)).squeeze(1)
        assert bool((t['istar'] >= 0).all()) and bool((t['istar'] < r['CX'].shape[1]).all())
        assert bool((r['c'] - at <= 2 * eb['ec']).all()), 'i* of tap %d' % l
        _within(cx[l], r['cxn'], eb['ecxn'], 'CX[n] of tap %d' % l)
        et = cc.term_bound(r['cxn'], eb['ecxn'])
        _within(terms[l], want_terms[l], torch.tensor(et, dtype=F64), 'term of tap %d' % l)
        e_loss += abs(WEIGHT * wl) * et
        # the gradient: the float64 formulas on the device's S, Z, i*, j*, norms, mu and CX[n]
        x, y = split(fa, shapes)[l], split(fb, shapes)[l]
        ref, pc = cc.grad64(x, y, t['mu'], r, t['istar'], t['jstar'], cx[l].cpu(), G * WEIGHT * wl, BAND, Z=t['Z'], na=t['na'], nb=t['nb'])
        _within(grads[l], ref, cc.grad_bound(r, pc, BAND, eb['rho']), 'gradient of tap %d' % l)
    _within(loss, want_loss, torch.tensor(e_loss + U * abs(float(want_loss)), dtype=F64), 'loss')


def _distances(fa, fb, shapes, lw):
    """-> (device, fp32 torch composition): the largest gradient difference from the float64 autograd of the composition, over its
    largest gradient element"""
    a64 = fa.to(F64).requires_grad_()
    (ref,) = torch.autograd.grad(G * composition(a64, fb.to(F64), shapes, lw, BAND, WEIGHT), a64)
    a32 = fa.cuda().requires_grad_()
    (g32,) = torch.autograd.grad(G * composition(a32, fb.cuda(), shapes, lw, BAND, WEIGHT), a32)
    a = fa.cuda().requires_grad_()
    (got,) = torch.autograd.grad(G * pkg('losses').contextual_loss(a, fb.cuda(), shapes, lw, BAND, WEIGHT), a)
    top = float(ref.abs().max())
    return float((got.cpu().to(F64) - ref).abs().max()) / top, float((g32.cpu().to(F64) - ref).abs().max()) / top


def test_end_to_end_against_float64_autograd_of_the_composition():
    """A case takes part if the float64 reference's own margins -- min_i (d_(2) - d_(1)) and the relative gap of the two largest CX_.j --
    exceed twice the derived S error bound: then no discrete choice of the device can differ from the reference's.  The bar: no farther
    from float64 than 4 x the fp32 torch composition on the same inputs (the factor covers another summation order in a K <= 256 chain)"""
    took = 0
    for case, kind in [(c, k) for c in SMALL for k in KINDS]:
        b, shapes, lw, _ = case
        fa, fb = _inputs(case, kind)
        taps = cc.forward64(fa, fb, shapes, lw, BAND, WEIGHT)[3]
        gap_d, gap_c = cc.margins64(taps)
        bound = max(float(e.max()) for e in cc.sim_bound(fa, fb, shapes))
        if not (gap_d > 2 * bound and gap_c > 2 * bound):
            print('%s %s: left out (margins %.2e, %.2e against 2 x %.2e)' % (case_id(case), kind, gap_d, gap_c, bound))
            continue
        took += 1
        ours, torchs = _distances(fa, fb, shapes, lw)
        print('%s %s: device %.3e, fp32 composition %.3e of the largest gradient element (margins %.2e, %.2e, S bound %.2e)'
              % (case_id(case), kind, ours, torchs, gap_d, gap_c, bound))
        assert ours <= 4 * torchs, (case_id(case), kind, ours, torchs)
    assert took >= 5, took


# ---- properties ---------------------------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits():
    Lm = pkg('losses')
    for case in (CASES[6], CASES[5]):
        fa, fb = (t.cuda() for t in _inputs(case, 'correlated'))
        outs = []
        for _ in range(2):
            a = fa.clone().requires_grad_()
            loss, terms, cx = Lm.contextual_loss(a, fb, case[1], case[2], BAND, WEIGHT, return_terms=True)
            loss.backward()
            outs.append((loss.detach(), terms, cx, a.grad) + Lm.contextual_similarity(a, fb, case[1]))
        assert all(torch.equal(x, y) for x, y in zip(*outs))
        assert float(outs[0][3].abs().max()) > 0


def test_one_point_gives_cx_one_and_a_zero_gradient():
    Lm = pkg('losses')
    case = CASES[3]
    fa, fb = (t.cuda() for t in _inputs(case, 'uniform'))
    a = fa.clone().requires_grad_()
    loss, terms, cx = Lm.contextual_loss(a, fb, case[1], return_terms=True)
    loss.backward()
    want = float(torch.tensor(-math.log1p(1e-5), dtype=F64).to(torch.float32))          # -log(1 + 1e-5), rounded once
    assert torch.equal(cx.cpu(), torch.ones(1, 1)) and float(loss.detach()) == want and float(terms[0]) == want
    assert torch.equal(a.grad, torch.zeros_like(a))


def test_equal_inputs_saturate_without_a_nan():
    Lm = pkg('losses')
    case = CASES[6]
    x = _inputs(case, 'uniform')[1].cuda()
    a = x.clone().requires_grad_()
    loss, terms, cx = Lm.contextual_loss(a, x.clone(), case[1], case[2], return_terms=True)
    loss.backward()
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(terms).all()) and bool(torch.isfinite(a.grad).all())
    assert abs(float(loss)) < 1e-3 and float(cx.min()) > 0.99


def test_one_nan_feature_gives_a_nan_term_without_a_fault():
    Lm = pkg('losses')
    b, shapes, lw, _ = CASES[6]
    fa, fb = (t.cuda() for t in _inputs(CASES[6], 'uniform'))
    clean = Lm.contextual_loss(fa, fb, shapes, lw, return_terms=True)
    for side in (0, 1):
        bad = [fa.clone(), fb.clone()]
        bad[side][1, 45 + 7] = float('nan')                        # inside the second tap
        a = bad[0].requires_grad_()
        loss, terms, cx = Lm.contextual_loss(a, bad[1], shapes, lw, return_terms=True)
        loss.backward()
        torch.cuda.synchronize()
        nan = torch.tensor([False, True, False], device='cuda')
        assert torch.equal(torch.isnan(terms), nan) and torch.equal(terms[~nan], clean[1][~nan]) and bool(torch.isnan(loss))
        assert bool(torch.isnan(cx[1, 1])) and torch.equal(cx[0], clean[2][0])


def test_zero_layer_weight_and_the_target_side():
    Lm = pkg('losses')
    b, shapes, _, _ = CASES[6]
    fa, fb = (t.cuda().requires_grad_() for t in _inputs(CASES[6], 'correlated'))
    loss = Lm.contextual_loss(fa, fb, shapes, (1.0, 0.0, 2.0))
    loss.backward()
    assert fb.grad is None
    ga = split(fa.grad, shapes)
    assert torch.equal(ga[1], torch.zeros_like(ga[1])) and float(ga[0].abs().max()) > 0 and float(ga[2].abs().max()) > 0


def test_contextual_loss_module_through_the_extractor():
    """ContextualLoss around a MaskedVGG against the same extractor followed by the fp32 composition, both from float64 autograd of
    the composition on the extractor's fp32 features: the 4 x bar on the feature gradient that enters VGGFunction.backward, and the image
    gradients next to each other"""
    Lm, ce = pkg('losses'), pkg('model_content_extractor')
    net = ce.MaskedVGG(0b00111, width_div=4, pretrained=False).cuda()
    lw = (0.5, 1.0, 2.0)
    mod = Lm.ContextualLoss(net, lw, BAND, WEIGHT).cuda()
    gen = torch.Generator().manual_seed(5)
    x, gt = (2 * torch.rand((2, 3, 16, 16), generator=gen) - 1 for _ in range(2))
    shapes = ce.tap_shapes(net, 16, 16)
    assert shapes == ((16, 16, 16), (32, 8, 8), (64, 4, 4))
    xd = x.cuda().requires_grad_()
    loss = mod(xd, gt.cuda())
    loss.backward()
    xr = x.cuda().requires_grad_()
    with torch.no_grad():
        fg = net(gt.cuda()).reshape(2, -1)
    fx = net(xr).reshape(2, -1)
    ref = composition(fx, fg, shapes, lw, BAND, WEIGHT)
    ref.backward()
    f64 = fx.detach().cpu().to(F64).requires_grad_()
    (g64,) = torch.autograd.grad(composition(f64, fg.cpu().to(F64), shapes, lw, BAND, WEIGHT), f64)
    f32 = fx.detach().clone().requires_grad_()
    (g32,) = torch.autograd.grad(composition(f32, fg, shapes, lw, BAND, WEIGHT), f32)
    fo = fx.detach().clone().requires_grad_()
    (go,) = torch.autograd.grad(Lm.contextual_loss(fo, fg, shapes, lw, BAND, WEIGHT), fo)
    top = float(g64.abs().max())
    ours, torchs = float((go.cpu().to(F64) - g64).abs().max()) / top, float((g32.cpu().to(F64) - g64).abs().max()) / top
    rel = float((xd.grad - xr.grad).abs().max() / xr.grad.abs().max())
    print('feature gradient: device %.3e, fp32 composition %.3e of its largest element; image gradients differ by %.3e; loss %g vs %g'
          % (ours, torchs, rel, float(loss), float(ref)))
    assert top > 0 and ours <= 4 * torchs
    assert float(xr.grad.abs().max()) > 0 and rel <= 1e-3 and abs(float(loss) - float(ref)) <= 1e-4 * abs(float(ref))


def test_forward_and_backward_are_capturable():
    """torch.cuda.graph captures contextual_loss forward + backward; three replays on new contents of the static inputs are bit-equal to
    eager calls on those contents"""
    Lm = pkg('losses')
    b, shapes, lw, relu = CASES[6]
    s_a, s_b = (torch.zeros(b, total_of(shapes), device='cuda') for _ in range(2))

    def run(fa, fb):
        a = fa.detach().requires_grad_()
        loss, terms, cx = Lm.contextual_loss(a, fb, shapes, lw, BAND, WEIGHT, return_terms=True)
        (da,) = torch.autograd.grad(loss, a)
        return loss.detach(), terms, cx, da
    s_a.copy_(_inputs(CASES[6], 'correlated')[0])
    s_b.copy_(_inputs(CASES[6], 'correlated')[1])
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
        fa, fb = (t.cuda() for t in cc.inputs(b, shapes, relu, 'correlated', seed=10 + rep))
        s_a.copy_(fa)
        s_b.copy_(fb)
        graph.replay()
        torch.cuda.synchronize()
        eager = run(fa, fb)
        assert all(torch.equal(x, y) for x, y in zip(out, eager)), rep
        assert float(out[3].abs().max()) > 0
