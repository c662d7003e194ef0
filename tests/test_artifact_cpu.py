"""CPU: the host side of the artifact-aware (LDL) loss: the two float64 restatements of artifact_cases.py
against each other and against the autograd of the composition with a detached map; the conditions the GPU comparison stands on,
for every case; the new entry points refuse every bad argument before they touch a GPU; the Python wrappers refuse CPU and fp64
tensors and bad window sizes."""
import ctypes as C

import pytest
import torch

from artifact_cases import (AMPS, CASES, F64, IDS, LOSS_BOUND, MAP_BOUND, NEAR_SHARE, case, composition, composition_loss, grad64, loss64,
                            map64, pkg, residuals64)

BADARG, TOOBIG, UNSUPPORTED = -1, -2, -3


@pytest.mark.parametrize('amp', AMPS)
@pytest.mark.parametrize('shape,K', CASES, ids=IDS)
def test_restatements_agree_and_the_cases_hold_their_conditions(shape, K, amp):
    """explicit mirrored indexing against reflect F.pad + unfold + torch.var, both float64; then what the GPU test assumes of the
    reference alone: few near ties, a mixed mask, and torch's own fp32 composition inside the bounds the kernels are held to"""
    sr, gt, ema, m, masked, near = case(shape, K, amp)
    c64 = composition(gt.to(F64), sr.to(F64), ema.to(F64), K)
    err = float((c64 - m).abs().max())
    share, frac = float(near.to(F64).mean()), float(masked.to(F64).mean())
    top = m.amax(dim=(1, 2, 3), keepdim=True)
    c32 = composition(gt, sr, ema, K)
    away = ~near.unsqueeze(1)
    d_map = float(((c32.to(F64) - m).abs() / top)[away.expand_as(m)].max())
    own32 = torch.sum(torch.abs(gt - sr), 1) < torch.sum(torch.abs(gt - ema), 1)            # the fp32 composition's own mask
    ref = loss64(sr, gt, map64(gt, sr, ema, K, mask=own32)[0])
    d_loss = float(((composition_loss(sr, gt, c32).to(F64) - ref).abs() / ref).max())
    print('%s K %d amp %g: restatement - composition %.3e; masked %.3f, near ties %.2e; fp32 composition: map %.3e of the maximum '
          '(bound %.1e), loss %.3e relative (bound %.1e)' % (shape, K, amp, err, frac, share, d_map, MAP_BOUND, d_loss, LOSS_BOUND))
    assert err <= 1e-12
    assert share <= NEAR_SHARE
    assert 0.2 < frac < 0.8
    assert d_map <= MAP_BOUND and d_loss <= LOSS_BOUND
    assert bool((top > 0).all())


@pytest.mark.parametrize('shape,K', [CASES[1], CASES[3], CASES[5]], ids=[IDS[1], IDS[3], IDS[5]])
def test_gradient_formula_is_the_autograd_of_the_composition_with_a_detached_map(shape, K):
    sr, gt, ema = (t.to(F64) for t in case(shape, K, 0.3)[:3])
    sr.requires_grad_()
    gt.requires_grad_()
    g = torch.linspace(0.5, 1.5, shape[0], dtype=F64)
    m = composition(gt, sr, ema, K)
    assert not m.requires_grad
    loss = composition_loss(sr, gt, m, 0.7)
    assert float((loss.detach() - loss64(sr.detach(), gt.detach(), m, 0.7)).abs().max()) <= 1e-12
    d_sr, d_gt = torch.autograd.grad((g * loss).sum(), (sr, gt))
    want = grad64(sr.detach(), gt.detach(), m, g, 0.7)
    print('%s K %d: formula - autograd %.3e (dsr), %.3e (dgt)' % (shape, K, float((want - d_sr).abs().max()), float((want + d_gt).abs().max())))
    assert float((want - d_sr).abs().max()) <= 1e-12 and float((want + d_gt).abs().max()) <= 1e-12


def test_tie_and_cancellation_properties_of_the_reference():
    """what the exact GPU properties mirror: ema == sr masks nothing (the comparison is strict), and neither does ema == gt (r_ema
    is 0, and r_sr < 0 never holds); an ema twice as far from gt as sr masks every pixel with r_sr > 0; a constant residual has a
    map of rounding size only"""
    sr, gt, ema = case(CASES[3][0], 7, 0.3)[:3]
    assert not bool(map64(gt, sr, sr, 7)[1].any())
    assert not bool(map64(gt, sr, gt, 7)[1].any())
    far = gt + 2 * (sr - gt)
    assert torch.equal(map64(gt, sr, far, 7)[1], residuals64(gt, sr, far)[0] > 0)
    flat = map64(gt, gt + 0.5, gt + 0.5, 7)[0]
    assert float(flat.max()) <= 1e-12


def test_every_bad_argument_is_refused_without_a_gpu():
    lib = pkg('_lib').lib()
    buf = (C.c_double * 8)()
    # non-null, 8-byte aligned pointers 16 MiB apart: every call here is refused, refused calls never read them, and nothing
    # reaches a launch
    p = C.cast(buf, C.c_void_p)
    q, r, s, t, u = (C.c_void_p(p.value + (i << 24)) for i in (1, 2, 3, 4, 5))
    nan, inf = float('nan'), float('inf')
    n_floats = lib.sisr_artifact_ws_floats(2, 40, 40)
    assert n_floats >= 2 * 2 * 40 * 40 and n_floats % 2 == 0
    assert lib.sisr_artifact_ws_floats(1, 4, 4) >= 2 * 16
    for bad in ((0, 4, 4), (-1, 4, 4), (1, 0, 4), (1, 4, -1)):
        assert lib.sisr_artifact_ws_floats(*bad) == BADARG, bad
    for bad in ((1, 1 << 16, 1 << 16), (1 << 20, 1 << 10, 1 << 10), (1100, 1 << 10, 1 << 10), ((1 << 31) - 1, (1 << 31) - 1, (1 << 31) - 1)):
        assert lib.sisr_artifact_ws_floats(*bad) == TOOBIG, bad
    good = dict(sr=p, gt=q, ema=r, N=2, C=3, H=40, W=40, ksize=7, weight=1.0, ws=s, map=t, loss=u, stream=None)
    for bad in (dict(sr=None), dict(gt=None), dict(ema=None), dict(ws=None), dict(map=None), dict(ws=C.c_void_p(s.value + 4)),
                dict(N=0), dict(N=-2), dict(H=0), dict(W=-1), dict(ksize=0), dict(ksize=1), dict(ksize=2), dict(ksize=8), dict(ksize=13),
                dict(ksize=-3), dict(weight=nan), dict(weight=inf)):
        assert lib.sisr_artifact_fwd(*dict(good, **bad).values()) == BADARG, bad
    for bad in (dict(C=0), dict(C=2), dict(C=4), dict(H=3), dict(W=3), dict(ksize=11, H=5), dict(ksize=3, W=1)):
        assert lib.sisr_artifact_fwd(*dict(good, **bad).values()) == UNSUPPORTED, bad
    for bad in (dict(H=1 << 16, W=1 << 16), dict(N=1 << 20, H=1 << 10, W=1 << 10), dict(N=700, H=1 << 10, W=1 << 10, C=3),
                dict(N=1100, H=1 << 10, W=1 << 10, C=1)):         # the last one: the workspace alone is too big
        assert lib.sisr_artifact_fwd(*dict(good, **bad).values()) == TOOBIG, bad
    good = dict(sr=p, gt=q, map=r, g=s, N=2, C=3, H=40, W=40, weight=1.0, dsr=t, dgt=u, stream=None)
    for bad in (dict(sr=None), dict(gt=None), dict(map=None), dict(g=None), dict(dsr=None, dgt=None), dict(N=0), dict(H=0), dict(W=0),
                dict(weight=nan), dict(weight=-inf)):
        assert lib.sisr_artifact_bwd(*dict(good, **bad).values()) == BADARG, bad
    for bad in (dict(C=2), dict(C=0)):
        assert lib.sisr_artifact_bwd(*dict(good, **bad).values()) == UNSUPPORTED, bad
    for bad in (dict(H=1 << 16, W=1 << 16), dict(N=1 << 20, H=1 << 10, W=1 << 10), dict(N=800, H=1 << 10, W=1 << 10)):
        assert lib.sisr_artifact_bwd(*dict(good, **bad).values()) == TOOBIG, bad


def test_python_wrappers_validate_and_refuse_cpu_and_fp64_tensors():
    Lm, top = pkg('losses'), pkg()
    assert top.artifact_loss is Lm.artifact_loss and top.artifact_map is Lm.artifact_map
    x = torch.zeros(2, 3, 16, 16)
    calls = (lambda a, b, c, **kw: Lm.artifact_loss(a, b, c, **kw), lambda a, b, c, **kw: Lm.artifact_map(b, a, c, **kw))
    for call in calls:
        with pytest.raises(RuntimeError):
            call(x, x, x)                                          # CPU tensors: no fallback
        for bad in (x.double(), x.half(), x.to(torch.bfloat16), None, x[:, :2], x[0], torch.zeros(2, 3, 16, 17), torch.zeros(0, 3, 16, 16)):
            for args in ((bad, x, x), (x, bad, x), (x, x, bad)):
                with pytest.raises(ValueError):
                    call(*args)
        for bad in (0, 1, 2, 8, 13, -7, 7.0, True, None):
            with pytest.raises(ValueError):
                call(x, x, x, ksize=bad)
        y = torch.zeros(1, 1, 3, 9)
        with pytest.raises(ValueError):
            call(y, y, y)                                          # H = P at the default window
        with pytest.raises(ValueError):
            call(y.transpose(2, 3), y.transpose(2, 3), y.transpose(2, 3), ksize=7)
        with pytest.raises(RuntimeError):
            call(y, y, y, ksize=5)                                 # a legal call: refused for the device alone
        with pytest.raises(RuntimeError):
            call(x.transpose(2, 3), x.transpose(2, 3), x.transpose(2, 3))      # strided is legal (made contiguous); CPU is not
    for bad in (dict(reduction='sum'), dict(weight=float('nan')), dict(weight=float('inf'))):
        with pytest.raises(ValueError):
            Lm.artifact_loss(x, x, x, **bad)
