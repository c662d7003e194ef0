"""CPU: the host side of the contextual loss: the gradient formulas of contextual_cases.py against the float64
autograd of the common PyTorch composition; torch's own fp32 composition stays inside the derived bounds, so they are not vacuous; the
entry points and the Python wrappers refuse every bad argument before they touch a GPU; the constants of _lib are the header's;
tap_shapes drives ContextualLoss up to the device check."""
import ctypes as C
import os
import re

import pytest
import torch

import contextual_cases as cc
from contextual_cases import BAND, CASES, F64, KINDS, case_id, composition, pkg, split

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BADARG, TOOBIG = -1, -2
BOTH = [(c, k) for c in CASES for k in KINDS]


def _id(ck):
    return case_id(ck[0]) + '-' + ck[1]


@pytest.mark.parametrize('ck', BOTH, ids=_id)
def test_gradient_formulas_are_the_autograd_of_the_composition(ck):
    case, kind = ck
    b, shapes, lw, relu = case
    fa, fb = cc.inputs(b, shapes, relu, kind)
    a = fa.to(F64).requires_grad_()
    loss = composition(a, fb.to(F64), shapes, lw, BAND, 1.5)
    (auto,) = torch.autograd.grad(0.7 * loss, a)
    want_loss, terms, cx, _ = cc.forward64(fa, fb, shapes, lw, BAND, 1.5)
    want = cc.loss_grad64(fa, fb, shapes, lw, BAND, 1.5, 0.7)
    top = float(auto.abs().max())
    err = float((want - auto).abs().max()) / (top if top > 0 else 1.0)
    print('%s %s: loss %.6g, formula - autograd %.3e of the largest gradient element %.3e' % (case_id(case), kind, float(loss.detach()), err, top))
    assert abs(float(want_loss) - float(loss.detach())) <= 1e-13 * max(abs(float(want_loss)), 1.0)     # -log(CX + 1e-5) cancels near CX = 1
    assert err <= 1e-12
    assert terms.shape == (len(shapes),) and cx.shape == (len(shapes), b)
    if max(h * w for _, h, w in shapes) > 1:
        assert top > 0                                               # neither input kind saturates
    else:
        assert top == 0 and float(cx.min()) == 1.0                   # P = 1: CX = 1 and a zero gradient


@pytest.mark.parametrize('ck', BOTH, ids=_id)
def test_torch_fp32_composition_is_inside_the_derived_bounds(ck):
    """the bounds the kernels are held to leave room for a correct fp32 evaluation: torch's own S stays inside sim_bound, and its
    fp32 rows (from its own S) inside row_bounds"""
    case, kind = ck
    b, shapes, lw, relu = case
    fa, fb = cc.inputs(b, shapes, relu, kind)
    worst_s = worst_z = worst_c = 0.0
    for x, y, (ref, _), bound in zip(split(fa, shapes), split(fb, shapes), cc.sim64(fa, fb, shapes), cc.sim_bound(fa, fb, shapes)):
        mu = y.mean(dim=(0, 2), keepdim=True)
        s32 = torch.bmm(torch.nn.functional.normalize(x - mu, dim=1).transpose(1, 2), torch.nn.functional.normalize(y - mu, dim=1))
        worst_s = max(worst_s, float(((s32.to(F64) - ref).abs() / bound.clamp_min(1e-300)).max()))
        d32 = 1 - s32
        r = cc.rows64(cc.d_of(s32), BAND)
        r['c'], r['istar'], r['cxn'] = cc.cols64(r['CX'])
        eb = cc.row_bounds(r, BAND)
        w32 = torch.exp((1 - d32 / (d32.min(dim=2, keepdim=True)[0] + cc.EPS)) / BAND)
        z32 = w32.sum(2)
        c32 = (w32 / z32.unsqueeze(2)).max(dim=1)[0]
        # torch sums Z in fp32: P more roundings than the kernel's double sum, which the comparison allows for
        worst_z = max(worst_z, float(((z32.to(F64) - r['Z']).abs() / (eb['eZ'] + x.shape[2] * cc.U * r['Z'])).max()))
        worst_c = max(worst_c, float(((c32.to(F64) - r['c']).abs() / (eb['ec'] + x.shape[2] * cc.U * r['c'])).max()))
    print('%s %s: torch fp32 uses %.3f of the S bound, %.3f of the Z bound, %.3f of the c bound' % (case_id(case), kind, worst_s, worst_z, worst_c))
    assert worst_s <= 1.0 and worst_z <= 1.0 and worst_c <= 1.0


def test_lib_constants_are_the_headers():
    L = pkg('_lib')
    hdr = open(os.path.join(ROOT, 'include', 'sisr_hip.h')).read()
    defs = {k: int(v) for k, v in re.findall(r'#define (SISR_CX_[A-Z0-9_]+) (\d+)', hdr)}
    assert defs == {'SISR_CX_MAX_POINTS': L.CX_MAX_POINTS, 'SISR_CX_WS_TABLES': L.CX_WS_TABLES, 'SISR_CX_WS_SIM': L.CX_WS_SIM,
                    'SISR_CX_WS_FWD': L.CX_WS_FWD, 'SISR_CX_WS_BWD': L.CX_WS_BWD}
    assert L.CX_MAX_POINTS == 2304


def _shapes(*taps):
    return (C.c_int32 * (3 * len(taps)))(*[v for s in taps for v in s])


def test_every_bad_argument_is_refused_without_a_gpu():
    Lb = pkg('_lib')
    lib = Lb.lib()
    buf = (C.c_double * 8)()
    # non-null, 16-byte aligned pointers 16 MiB apart: every call here is refused, refused calls never read them, nothing reaches a launch
    base = (C.cast(buf, C.c_void_p).value + 15) & ~15
    p, q, r, s, t, u, v = (C.c_void_p(base + (i << 24)) for i in range(1, 8))
    one, three = _shapes((4, 2, 2)), _shapes((4, 2, 2), (8, 1, 1), (2, 3, 1))
    nine = _shapes(*[(1, 1, 1)] * 9)
    w = (C.c_float * 9)(*[1.0] * 9)
    # the size queries: B = 2, P = 4, 1, 3; C = 4, 8, 2
    assert lib.sisr_cx_ws_bytes(2, 3, three, Lb.CX_WS_TABLES) == 4 * (14 + 7 * 2 * 8)
    assert lib.sisr_cx_ws_bytes(2, 3, three, Lb.CX_WS_SIM) == 4 * 2 * (16 + 1 + 9)
    fwd = lib.sisr_cx_ws_bytes(2, 3, three, Lb.CX_WS_FWD)
    assert fwd >= 4 * 2 * 26 + 8 * 6 and fwd % 8 == 0
    assert lib.sisr_cx_ws_bytes(2, 3, three, Lb.CX_WS_BWD) == 4 * (2 * 26 + 2 * 30)
    # conv2_2 at HR 96^2, B 16: the similarity is 340 MB
    assert lib.sisr_cx_ws_bytes(16, 1, _shapes((128, 48, 48)), Lb.CX_WS_SIM) == 4 * 16 * 2304 * 2304
    for bad in ((0, 1, one), (-1, 1, one), (2, 0, one), (2, 9, nine), (2, 1, None), (2, 1, _shapes((0, 2, 2))), (2, 1, _shapes((4, -1, 2))),
                (2, 1, _shapes((4, 2, 0)))):
        assert lib.sisr_cx_ws_bytes(*bad, 0) == BADARG, bad[:2]
    assert lib.sisr_cx_ws_bytes(2, 1, one, 4) == BADARG and lib.sisr_cx_ws_bytes(2, 1, one, -1) == BADARG
    assert lib.sisr_cx_ws_bytes(1, 1, _shapes((4, 49, 48)), 0) == TOOBIG and lib.sisr_cx_ws_bytes(1, 1, _shapes((4, 48, 48)), 0) > 0
    good = dict(fa=p, fb=q, B=2, total=16, n=1, shapes=one, tab=r, sim=s, stream=None)
    for bad in (dict(fa=None), dict(fb=None), dict(tab=None), dict(sim=None), dict(tab=C.c_void_p(r.value + 2)), dict(B=0), dict(n=0),
                dict(n=9, shapes=nine, total=9), dict(total=15), dict(total=0), dict(shapes=None), dict(shapes=_shapes((4, 0, 4)))):
        assert lib.sisr_cx_sim(*dict(good, **bad).values()) == BADARG, bad
    assert lib.sisr_cx_sim(*dict(good, shapes=_shapes((1, 49, 48)), total=49 * 48).values()) == TOOBIG
    good = dict(fa=p, fb=q, B=2, total=30, n=3, shapes=three, lw=w, h=0.5, weight=1.0, tab=r, ws=s, terms=t, cx=u, loss=v, stream=None)
    for bad in (dict(fa=None), dict(fb=None), dict(lw=None), dict(tab=None), dict(ws=None), dict(cx=None), dict(loss=None), dict(shapes=None),
                dict(ws=C.c_void_p(s.value + 4)), dict(B=0), dict(B=-3), dict(n=0), dict(n=-1), dict(n=9, shapes=nine, total=9), dict(total=29),
                dict(total=31), dict(h=0.0), dict(h=-0.5), dict(h=float('nan')), dict(h=float('inf')),
                dict(shapes=_shapes((4, 2, 2), (8, 0, 1), (2, 3, 1)))):
        assert lib.sisr_cx_fwd(*dict(good, **bad).values()) == BADARG, bad
    good = dict(fa=p, fb=q, tab=r, cx=u, g=v, B=2, total=30, n=3, shapes=three, lw=w, h=0.5, weight=1.0, ws=s, dfa=t, stream=None)
    for bad in (dict(fa=None), dict(fb=None), dict(tab=None), dict(cx=None), dict(g=None), dict(lw=None), dict(ws=None), dict(dfa=None),
                dict(shapes=None), dict(ws=C.c_void_p(s.value + 8)), dict(B=0), dict(n=0), dict(n=9, shapes=nine, total=9), dict(total=29),
                dict(h=0.0), dict(h=float('nan')), dict(h=-1.0)):
        assert lib.sisr_cx_bwd(*dict(good, **bad).values()) == BADARG, bad


def test_python_wrappers_validate_and_refuse_cpu_tensors():
    Lm, top = pkg('losses'), pkg()
    assert top.contextual_loss is Lm.contextual_loss and top.contextual_similarity is Lm.contextual_similarity
    assert top.ContextualLoss is Lm.ContextualLoss
    shapes = ((4, 2, 2), (2, 3, 1))
    x = torch.zeros(2, 22)
    with pytest.raises(RuntimeError):
        Lm.contextual_loss(x, x, shapes)                            # CPU tensors: no fallback
    with pytest.raises(RuntimeError):
        Lm.contextual_similarity(x, x, shapes)
    for bad in (((4, 2, 2),), ((4, 2, 2), (2, 3, 2)), ((1, 1, 1),) * 9, ((4, 2, 2), (2, 3, 0), (1, 1, 6)), ((4, 2), (2, 3, 1)), (), 7,
                ((4, 2, 2), (2, -3, -1))):
        with pytest.raises(ValueError):
            Lm.contextual_loss(x, x, bad)
        with pytest.raises(ValueError):
            Lm.contextual_similarity(x, x, bad)
    for bad in (x.double(), x.half(), x.to(torch.bfloat16), None, torch.zeros(2, 23), torch.zeros(3, 22), torch.zeros(0, 22), torch.zeros(2, 2, 11)):
        with pytest.raises(ValueError):
            Lm.contextual_loss(bad, x, shapes)
        with pytest.raises(ValueError):
            Lm.contextual_loss(x, bad, shapes)
        with pytest.raises(ValueError):
            Lm.contextual_similarity(x, bad, shapes)
    big = torch.zeros(1, 3 * 49 * 48)
    with pytest.raises(ValueError, match='deeper tap or pool'):
        Lm.contextual_loss(big, big, ((3, 49, 48),))                # P = 2352 is above the cap
    with pytest.raises(ValueError, match='deeper tap or pool'):
        Lm.contextual_similarity(big, big, ((3, 49, 48),))
    for bad in (dict(band_width=0.0), dict(band_width=-0.5), dict(band_width=float('nan')), dict(band_width=float('inf')),
                dict(band_width=1e-60), dict(layer_weights=(1.0,)), dict(layer_weights=(1.0, 1.0, 1.0)), dict(layer_weights=(1.0, float('nan'))),
                dict(weight=float('inf'))):
        with pytest.raises(ValueError):
            Lm.contextual_loss(x, x, shapes, **bad)
    with pytest.raises(ValueError, match='band_width'):
        Lm.ContextualLoss(pkg('model_content_extractor').identity(), band_width=0.0)


def test_tap_shapes_drive_the_module_up_to_the_device_check():
    """a width_div extractor whose forward is replaced by host zeros of its own output size: the module takes the tap shapes from the
    extractor's layers, passes every argument check and is stopped by the device check of contextual_loss; with a feature vector of
    another size it is the argument check that refuses"""
    Lm, ce = pkg('losses'), pkg('model_content_extractor')

    class Host(ce.MaskedVGG):
        extra = 0

        def forward(self, x):
            return torch.zeros(x.shape[0], sum(c * h * w for c, h, w in ce.tap_shapes(self, x.shape[2], x.shape[3])) + self.extra)
    net = Host(0b01100, width_div=4, pretrained=False)
    assert ce.tap_shapes(net, 32, 32) == ((64, 8, 8), (128, 4, 4))
    mod = Lm.ContextualLoss(net, (1.0, 0.5), 0.25, 2.0, input_norm=True, range_norm=True)
    x, gt = torch.zeros(2, 3, 32, 32).requires_grad_(), torch.zeros(2, 3, 32, 32)
    with pytest.raises(RuntimeError, match='contextual_loss input fa'):
        mod(x, gt)
    with pytest.raises(ValueError, match='one layer weight per tap'):
        Lm.ContextualLoss(net, (1.0,))(x, gt)
    with pytest.raises(ValueError, match='deeper tap or pool'):
        mod(torch.zeros(1, 3, 400, 400), torch.zeros(1, 3, 400, 400))      # conv3_4 of a 400^2 image: 10000 points
    net.extra = 1
    with pytest.raises(ValueError, match='elements per sample'):
        mod(x, gt)
    with pytest.raises(RuntimeError):
        Lm.ContextualLoss(ce.MaskedVGG(0b01100, width_div=4, pretrained=False))(x, gt)      # the real extractor refuses CPU images itself
