"""GPU: the artifact-aware (LDL) loss (csrc/artifact.hip, losses.artifact_loss / artifact_map) against the float64
restatements of artifact_cases.py, through the C entry points (guards around every output and the workspace, two launches with
identical bits) and through the Python surface.

Bounds (artifact_cases.py).  The mask is compared element by element: it may differ from the restatement's only where
|r_sr - r_ema| <= NEAR = 1e-6 (the fp32 roundings of the two residual sums for values up to about 1); the share of such pixels is
asserted to be at most 1e-3 per case (0 on all cases but one, 4.1e-4 there).  Away from them |m - m64| <= MAP_BOUND max(m64[n]) with
MAP_BOUND = 9.8e-7 = 8 x the largest distance (1.223e-7) of torch's own fp32 composition from float64 on these cases on a CPU.  The
loss is compared, relative, with the float64 loss on the DEVICE's own mask, so no element is left out: LOSS_BOUND = 6e-7.  The
gradients: against the float64 formula on the device's own map to four fp32 roundings, and against the float64 autograd of the
composition with a detached map to MAP_BOUND of the sample's largest gradient, away from near ties."""
import pytest
import torch

from artifact_cases import (AMPS, CASES, F64, GRAD_ROUNDINGS, IDS, LOSS_BOUND, MAP_BOUND, NEAR, NEAR_SHARE, case, composition,
                            composition_loss, grad64, inputs, loss64, map64, pkg, residuals64)
from gpu_helpers import Buf, run2

pytestmark = pytest.mark.gpu
RAGGED = CASES[3]                                # (1, 3, 33, 65), K 7: both axes past a tile edge by one


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _forward_entry(sr, gt, ema, K, weight=1.0, with_loss=True):
    """-> (map [N, 1, H, W], loss [N] or None) of device tensors through sisr_artifact_fwd, launched twice: status 0, guards of the
    map, the loss and the workspace intact, identical bits"""
    lib = pkg('_lib').lib()
    n, c, h, w = sr.shape
    ws = Buf(lib.sisr_artifact_ws_floats(n, h, w))
    amap, loss = Buf(n * h * w), Buf(n)
    call = lambda: lib.sisr_artifact_fwd(sr.data_ptr(), gt.data_ptr(), ema.data_ptr(), n, c, h, w, K, weight, ws.ptr(), amap.ptr(),   # noqa: E731
                                         loss.ptr() if with_loss else None, _stream())
    run2(call, [amap, loss, ws])
    if not with_loss:
        assert bool((loss.body == loss.fill).all())
    return amap.body.view(n, 1, h, w).clone(), loss.body.clone() if with_loss else None


def _check_map(got, sr, gt, ema, K, what):
    """the device map against float64, element by element -> the device's mask"""
    m64, masked64 = map64(gt, sr, ema, K)
    r_sr, r_ema = residuals64(gt, sr, ema)
    near = (r_sr - r_ema).abs() <= NEAR
    got = got.cpu().to(F64)
    masked = got[:, 0] == 0
    differs = masked != masked64
    share = float(near.to(F64).mean())
    top = m64.amax(dim=(1, 2, 3), keepdim=True)
    err = ((got - m64).abs() / top)[:, 0][~near]
    worst = float(err.max()) if err.numel() else 0.0
    print('%s: masked %.3f, %d of %d mask elements differ (near-tie share %.2e), max |m - m64| / max m64 away from ties %.3e (bound %.1e)'
          % (what, float(masked.to(F64).mean()), int(differs.sum()), masked.numel(), share, worst, MAP_BOUND))
    assert share <= NEAR_SHARE                                     # the condition of the comparison, asserted
    assert not bool((differs & ~near).any()), 'a mask element differs away from a tie'
    assert worst <= MAP_BOUND
    return masked


@pytest.mark.parametrize('amp', AMPS)
@pytest.mark.parametrize('shape,K', CASES, ids=IDS)
def test_map_and_loss_match_float64(shape, K, amp):
    sr, gt, ema = case(shape, K, amp)[:3]
    got, loss = _forward_entry(sr.cuda(), gt.cuda(), ema.cuda(), K, 0.75)
    masked = _check_map(got, sr, gt, ema, K, 'map %s K %d amp %g' % (shape, K, amp))
    ref = loss64(sr, gt, map64(gt, sr, ema, K, mask=masked)[0], 0.75)
    rel = float(((loss.cpu().to(F64) - ref).abs() / ref).max())
    print('loss %s K %d amp %g: %s, relative error %.3e (bound %.1e)' % (shape, K, amp, loss.tolist(), rel, LOSS_BOUND))
    assert rel <= LOSS_BOUND
    only_map = _forward_entry(sr.cuda(), gt.cuda(), ema.cuda(), K, with_loss=False)[0]
    assert torch.equal(only_map, got)                              # the map-only call: the same map, the loss untouched


@pytest.mark.parametrize('shape,K', [CASES[1], CASES[3], CASES[4], CASES[5]], ids=[IDS[1], IDS[3], IDS[4], IDS[5]])
def test_backward(shape, K):
    Lm, lib = pkg('losses'), pkg('_lib').lib()
    sr, gt, ema, _, _, near = case(shape, K, 0.3)
    n, c, h, w = shape
    g = torch.linspace(0.5, 1.5, n)
    srd, gtd, emad = (t.cuda().requires_grad_() for t in (sr, gt, ema))
    loss, amap = Lm.artifact_loss(srd, gtd, emad, K, weight=0.75, reduction='none', return_map=True)
    assert loss.shape == (n,) and loss.requires_grad and not amap.requires_grad
    (g.cuda() * loss).sum().backward()
    assert emad.grad is None
    assert torch.equal(gtd.grad, -srd.grad)                        # bit for bit
    # the float64 formula on the device's own map
    want = grad64(sr, gt, amap.cpu(), g, 0.75)
    err = (srd.grad.cpu().to(F64) - want).abs()
    ratio = float((err / want.abs().clamp_min(1e-300)).max())
    print('backward %s K %d: max |dsr - formula| / |formula| %.3e (bound %.3e)' % (shape, K, ratio, GRAD_ROUNDINGS))
    assert bool((err <= GRAD_ROUNDINGS * want.abs()).all())
    assert torch.equal(srd.grad == 0, (amap == 0).expand_as(srd.grad) | (srd == gtd))
    # the float64 autograd of the composition with a detached map
    s64, g64, e64 = sr.to(F64).requires_grad_(), gt.to(F64).requires_grad_(), ema.to(F64)
    auto, auto_gt = torch.autograd.grad((g.to(F64) * composition_loss(s64, g64, composition(g64, s64, e64, K), 0.75)).sum(), (s64, g64))
    top = auto.abs().amax(dim=(1, 2, 3), keepdim=True)
    away = (~near).unsqueeze(1).expand_as(auto)
    d_sr = float(((srd.grad.cpu().to(F64) - auto).abs() / top)[away].max())
    d_gt = float(((gtd.grad.cpu().to(F64) - auto_gt).abs() / top)[away].max())
    print('backward %s K %d: against float64 autograd, of the largest gradient: dsr %.3e, dgt %.3e (bound %.1e)' % (shape, K, d_sr, d_gt, MAP_BOUND))
    assert d_sr <= MAP_BOUND and d_gt <= MAP_BOUND
    # a call that needs one gradient writes that one: the autograd function, then the entry point with guards
    for need_sr, need_gt in ((True, False), (False, True)):
        a, b = sr.cuda().requires_grad_(need_sr), gt.cuda().requires_grad_(need_gt)
        (g.cuda() * Lm.artifact_loss(a, b, ema.cuda(), K, weight=0.75, reduction='none')).sum().backward()
        assert (a.grad is not None) == need_sr and (b.grad is not None) == need_gt
        assert torch.equal(a.grad if need_sr else b.grad, srd.grad if need_sr else gtd.grad)
        out, gd = Buf(sr.numel()), g.cuda()
        call = lambda: lib.sisr_artifact_bwd(a.data_ptr(), b.data_ptr(), amap.data_ptr(), gd.data_ptr(), n, c, h, w, 0.75,   # noqa: E731
                                             out.ptr() if need_sr else None, None if need_sr else out.ptr(), _stream())
        run2(call, [out])
        assert torch.equal(out.body.view(shape), srd.grad if need_sr else gtd.grad)


def test_equal_images_give_exact_zeros():
    Lm = pkg('losses')
    sr, gt, ema = (t.cuda() for t in inputs(RAGGED[0], 0.3))
    a, b = gt.clone().requires_grad_(), gt.clone().requires_grad_()
    loss, amap = Lm.artifact_loss(a, b, ema, reduction='none', return_map=True)
    loss.sum().backward()
    for t in (loss, amap, a.grad, b.grad):
        assert torch.equal(t, torch.zeros_like(t)), 'not exactly zero (or a NaN)'


def test_tie_rule_and_masks_that_are_known_exactly():
    """ema is sr: every comparison is a tie and nothing is masked; ema == gt: r_ema is 0 and nothing is masked either, the same bits;
    an ema twice as far from gt as sr: every pixel with r_sr > 0 is masked"""
    Lm = pkg('losses')
    shape, K = RAGGED
    sr, gt, _ = inputs(shape, 0.3)
    srd, gtd = sr.cuda(), gt.cuda()
    m_tie = Lm.artifact_map(gtd, srd, srd, K)
    want = map64(gt, sr, sr, K, mask=torch.zeros(shape[0], shape[2], shape[3], dtype=torch.bool))[0]
    err = float(((m_tie.cpu().to(F64) - want).abs() / want.amax(dim=(1, 2, 3), keepdim=True)).max())
    print('ema is sr: max |m - m64| / max m64 %.3e (bound %.1e), smallest value %.3e' % (err, MAP_BOUND, float(m_tie.min())))
    assert err <= MAP_BOUND and float(m_tie.min()) > 0
    assert torch.equal(Lm.artifact_map(gtd, srd, gtd, K), m_tie)
    far = gt + 2 * (sr - gt)
    r_sr, r_far = residuals64(gt, sr, far)
    assert bool(((r_far - r_sr) > NEAR)[r_sr > NEAR].all())       # away from ties wherever sr is away from gt
    m_far = Lm.artifact_map(gtd, srd, far.cuda(), K).cpu()
    assert bool((m_far[:, 0][r_sr > NEAR] == 0).all())


def test_constant_residual_and_a_large_offset():
    """sr = gt + 0.5: r_sr is 1.5 up to the rounding of the sum, so both variances are of rounding size -- a difference of raw moments
    in fp32 gives about 1e-9 here.  All three images + 100: the residuals, and so the map, of the shifted fp32 images"""
    Lm = pkg('losses')
    shape, K = RAGGED
    sr, gt, ema = inputs(shape, 0.3)
    flat = Lm.artifact_map(gt.cuda(), (gt + 0.5).cuda(), (gt + 0.5).cuda(), K)
    print('constant residual: max m %.3e (bound 1e-12)' % float(flat.max()))
    assert float(flat.max()) <= 1e-12 and not bool(torch.isnan(flat).any())
    s100, g100, e100 = sr + 100, gt + 100, ema + 100
    _check_map(Lm.artifact_map(g100.cuda(), s100.cuda(), e100.cuda(), K), s100, g100, e100, K, 'offset 100')


def test_weight_reduction_and_the_map_only_call():
    Lm, top = pkg('losses'), pkg()
    shape, K = CASES[1]
    sr, gt, ema = (t.cuda() for t in inputs(shape, 0.3))

    def run(weight):
        a, b = sr.clone().requires_grad_(), gt.clone().requires_grad_()
        loss = Lm.artifact_loss(a, b, ema, K, weight=weight, reduction='none')
        loss.sum().backward()
        return loss.detach(), a.grad, b.grad
    one = run(1.0)
    for weight in (2.0, 0.5, -4.0):                                # powers of two: exactly linear
        assert all(torch.equal(x, weight * y) for x, y in zip(run(weight), one))
    for x, y in zip(run(3.0), one):                                # any weight: linear to the roundings of both sides (six at most)
        assert bool(((x - 3.0 * y).abs() <= 6 * 2.0 ** -24 * (3.0 * y).abs()).all())
    assert all(torch.equal(x, torch.zeros_like(x)) for x in run(0.0))
    mean = Lm.artifact_loss(sr, gt, ema, K)
    assert mean.shape == () and mean.dtype == torch.float32 and torch.equal(mean, one[0].mean())
    loss, amap = top.artifact_loss(sr.requires_grad_(), gt, ema, K, return_map=True)
    only = top.artifact_map(gt, sr, ema, K)
    assert torch.equal(only, amap) and amap.shape == (shape[0], 1) + shape[2:]
    assert loss.requires_grad and not amap.requires_grad and not only.requires_grad and only.grad_fn is None
    # strided inputs are made contiguous
    wide = torch.zeros(shape[:3] + (2 * shape[3],), device='cuda')
    wide[..., ::2] = sr.detach()
    assert torch.equal(Lm.artifact_map(gt, wide[..., ::2], ema, K), only)


def test_one_nan_pixel_stays_in_its_sample():
    """the patch weight is a whole-sample statistic: every pixel of that sample that is not masked becomes NaN (a masked one is
    set to exactly 0 after the product, as upstream), its loss is NaN, and the other sample keeps its bits"""
    Lm = pkg('losses')
    shape, K = (2, 3, 33, 65), 7
    sr, gt, ema = (t.cuda() for t in inputs(shape, 0.3))
    clean_loss, clean = Lm.artifact_loss(sr, gt, ema, K, reduction='none', return_map=True)
    bad = sr.clone()
    bad[1, 0, 17, 64] = float('nan')
    loss, amap = Lm.artifact_loss(bad, gt, ema, K, reduction='none', return_map=True)
    assert torch.equal(amap[0], clean[0]) and torch.equal(loss[0], clean_loss[0])
    unmasked = clean[1] != 0
    unmasked[0, 17, 64] = True                                     # r_sr is NaN there: the comparison is false
    assert torch.equal(torch.isnan(amap[1]), unmasked) and bool((amap[1][~unmasked] == 0).all())
    assert bool(torch.isnan(loss[1]))


def test_forward_and_backward_are_capturable():
    """torch.cuda.graph captures artifact_loss forward + backward with ema a static input; three replays on new contents of the
    static inputs are bit-equal to eager calls on those contents"""
    Lm = pkg('losses')
    shape, K = CASES[5]
    s_sr, s_gt, s_ema = (torch.zeros(shape, device='cuda') for _ in range(3))

    def run(sr, gt, ema):
        a, b = sr.detach().requires_grad_(), gt.detach().requires_grad_()
        loss, amap = Lm.artifact_loss(a, b, ema, K, weight=0.75, return_map=True)
        da, db = torch.autograd.grad(loss, (a, b))
        return loss.detach(), amap, da, db
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            run(s_sr, s_gt, s_ema)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run(s_sr, s_gt, s_ema)
    for rep in range(3):
        sr, gt, ema = (t.cuda() for t in inputs(shape, 0.3, seed=10 + 3 * rep))
        for dst, src in ((s_sr, sr), (s_gt, gt), (s_ema, ema)):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        eager = run(sr, gt, ema)
        assert all(torch.equal(x, y) for x, y in zip(out, eager)), rep
        assert float(out[0]) > 0 and float(out[1].max()) > 0
