"""GPU: losses.image_loss / ssim_loss / l1_loss / charbonnier_loss (csrc/image_loss.hip), forward and backward, against the
definition evaluated in float64 on the CPU from the same fp32 inputs, with the gradients from torch autograd:

    loss[n] = w_ssim (1 - SSIM[n]) + w_pix mean_{C',H',W'} rho(a - b),   rho = |d| / sqrt(d^2 + eps^2) / d^2

on the crop / luma view, SSIM with the separable 11-tap Gaussian (sigma 1.5) through F.conv2d at the "valid" positions.

Inputs and definition: image_cases.py, shared with test_gpu_metrics.py (a smooth pattern per image and plane plus noise whose
strength grows along x, never constant: a != b everywhere, so the L1 sign is never ambiguous).
Shapes: (1, 1, 11, 11) is one window position that every pixel's gradient comes from, (2, 3, 13, 17) a 3 x 7 region inside one tile, (2, 3, 45, 70) ragged tiles in both axes with a
backward halo that crosses tile seams, (1, 3, 96, 192) 6 x 6 position tiles and the 16th / 17th row and 32nd / 33rd column seams.
The upstream gradient differs from image to image (reduction='none', (loss * g).sum()).

Bounds.  Forward: |loss - ref| <= 2e-5 absolute (the project's SSIM bound; both terms are O(1) here).  Gradient:
max|grad - ref| <= 1e-4 max|ref| for da and for db: evaluating the same formula in fp32 instead of fp64 moves the gradient by at
most 8.6e-6 of max|ref| on these inputs, while the smallest slip tried (one window position dropped at a corner, a centre or a
tile seam) moves it by at least 1.7e-2 and a one-pixel shift by more than 1."""
import functools

import pytest
import torch
import torch.nn.functional as F

from gpu_helpers import pkg
from helpers import grads_close
from image_cases import WINDOW, _definition, _images

pytestmark = pytest.mark.gpu

FWD_TOL = 2e-5
GRAD_TOL = 1e-4

SHAPES = [(1, 1, 11, 11), (2, 3, 13, 17), (2, 3, 45, 70), (1, 3, 96, 192)]
VIEWS = [(0, False), (2, False), (4, True)]
CONFIGS = {                                  # name -> keyword arguments of image_loss
    'ssim': dict(ssim_weight=1.0, pixel_weight=0.0),
    'l1': dict(ssim_weight=0.0, pixel_weight=1.0, pixel='l1'),
    'charbonnier+ssim': dict(ssim_weight=1.0, pixel_weight=1.0, pixel='charbonnier', eps=1e-3),
    'mse': dict(ssim_weight=0.0, pixel_weight=1.0, pixel='mse'),
}


def _least(cfg):
    return WINDOW if CONFIGS[cfg]['ssim_weight'] != 0.0 else 1


VALUE_CASES = [(s, crop, luma, cfg) for s in SHAPES for crop, luma in VIEWS for cfg in CONFIGS
               if min(s[2], s[3]) - 2 * crop >= _least(cfg)]


def _upstream(n):
    """a different upstream gradient for every image"""
    return 1.0 + 0.5 * torch.arange(n, dtype=torch.float64)


@functools.lru_cache(maxsize=None)
def _reference(shape, crop, luma, cfg):
    """float64 on the CPU -> (loss [N], da, db) for the upstream gradient _upstream(N); never modified"""
    a, b = (t.double().requires_grad_() for t in _images(shape))
    loss = _definition(a, b, crop_border=crop, luma=luma, **CONFIGS[cfg])[0]
    da, db = torch.autograd.grad((loss * _upstream(shape[0])).sum(), (a, b))
    return loss.detach(), da, db


def _fused(shape, crop, luma, cfg, seed=0, want_b=True):
    """forward + backward on the device -> (loss [N], da, db or None)"""
    Lo = pkg('losses')
    a, b = (t.cuda() for t in _images(shape, seed))
    a.requires_grad_()
    b.requires_grad_(want_b)
    loss = Lo.image_loss(a, b, crop_border=crop, luma=luma, reduction='none', **CONFIGS[cfg])
    (loss * _upstream(shape[0]).float().cuda()).sum().backward()
    return loss.detach(), a.grad, b.grad


def _grad_err(got, want):
    return float((got.double().cpu() - want).abs().max() / want.abs().max())


@pytest.mark.parametrize('shape,crop,luma,cfg', VALUE_CASES)
def test_loss_and_gradients_match_the_float64_definition(shape, crop, luma, cfg):
    want, want_da, want_db = _reference(shape, crop, luma, cfg)
    loss, da, db = _fused(shape, crop, luma, cfg)
    assert loss.shape == (shape[0],) and loss.dtype == torch.float32 and loss.is_cuda
    assert da.shape == shape and db.shape == shape
    e_fwd = float((loss.double().cpu() - want).abs().max())
    e_a, e_b = _grad_err(da, want_da), _grad_err(db, want_db)
    print('image_loss %s crop %d luma %d %s: loss err %.3g, da err %.3g, db err %.3g of max|ref|' % (shape, crop, luma, cfg, e_fwd, e_a, e_b))
    assert e_fwd <= FWD_TOL
    assert e_a <= GRAD_TOL and e_b <= GRAD_TOL


@pytest.mark.parametrize('pixel', ['l1', 'charbonnier', 'mse'])
@pytest.mark.parametrize('crop,luma', [(0, False), (1, True)])
def test_pixel_only_path_takes_a_view_smaller_than_the_window(pixel, crop, luma):
    Lo = pkg('losses')
    shape = (1, 3, 5, 7)
    a0, b0 = _images(shape)
    a64, b64 = (t.double().requires_grad_() for t in (a0, b0))
    want = _definition(a64, b64, pixel=pixel, crop_border=crop, luma=luma)[0]
    want_da, want_db = torch.autograd.grad(want.sum(), (a64, b64))
    a, b = a0.cuda().requires_grad_(), b0.cuda().requires_grad_()
    loss = Lo.image_loss(a, b, pixel=pixel, crop_border=crop, luma=luma)
    assert loss.shape == ()
    loss.backward()
    assert abs(float(loss) - float(want.mean())) <= FWD_TOL
    assert _grad_err(a.grad, want_da) <= GRAD_TOL and _grad_err(b.grad, want_db) <= GRAD_TOL


@pytest.mark.parametrize('shape,crop,luma', [((2, 3, 45, 70), 2, False), ((1, 3, 96, 192), 4, True), ((2, 3, 13, 17), 1, False)])
def test_cropped_border_gets_exact_zeros_from_a_dirty_allocator(shape, crop, luma):
    """the gradients are torch.empty: blocks that held NaNs are handed back to the backward, which must write every element"""
    Lo = pkg('losses')
    for cfg in ('charbonnier+ssim', 'l1'):
        a, b = (t.cuda().requires_grad_() for t in _images(shape))
        loss = Lo.image_loss(a, b, crop_border=crop, luma=luma, **CONFIGS[cfg])
        dirty = [torch.full(shape, float('nan'), device='cuda') for _ in range(2)]
        del dirty                                    # two free blocks of the gradients' size, full of NaNs
        loss.backward()
        for grad in (a.grad, b.grad):
            assert bool(torch.isfinite(grad).all())
            inner = torch.zeros(shape, dtype=torch.bool, device='cuda')
            inner[:, :, crop:shape[2] - crop, crop:shape[3] - crop] = True
            assert bool((grad[~inner] == 0).all())
            assert bool((grad[inner] != 0).any())


def test_luma_gradients_are_the_luma_gradient_times_the_coefficients():
    shape = (1, 3, 96, 192)
    for cfg in ('charbonnier+ssim', 'ssim'):
        _, da, db = _fused(shape, 4, True, cfg)
        for grad in (da, db):
            g = grad.double().cpu()
            nz = g[:, 0] != 0
            assert int(nz.sum()) == 88 * 184
            assert float((g[:, 1][nz] / g[:, 0][nz] - 0.587 / 0.299).abs().max()) <= 1e-6
            assert float((g[:, 2][nz] / g[:, 0][nz] - 0.114 / 0.299).abs().max()) <= 1e-6


@pytest.mark.parametrize('shape', [(2, 3, 45, 70), (1, 1, 11, 11)])
def test_equal_images_give_zero_loss_and_a_vanishing_gradient(shape):
    Lo = pkg('losses')
    a = _images(shape)[0].cuda().requires_grad_()
    b = a.detach().clone()
    loss = Lo.ssim_loss(a, b, reduction='none')
    (loss * _upstream(shape[0]).float().cuda()).sum().backward()
    scale = float(_reference(shape, 0, False, 'ssim')[1].abs().max())        # the unequal pair of the same shape
    print('image_loss equal images %s: loss %.3g, max|da| %.3g of the unequal pair\'s' % (shape, float(loss.abs().max()), float(a.grad.abs().max()) / scale))
    assert float(loss.abs().max()) <= 1e-6
    assert float(a.grad.abs().max()) <= 1e-4 * scale


def test_only_the_gradient_asked_for_is_computed():
    shape, view = (2, 3, 45, 70), (2, False, 'charbonnier+ssim')
    loss2, da2, db2 = _fused(shape, *view)
    loss1, da1, db1 = _fused(shape, *view, want_b=False)
    assert db1 is None and torch.equal(da1, da2) and torch.equal(loss1, loss2)
    Lo = pkg('losses')
    a, b = (t.cuda() for t in _images(shape))
    b.requires_grad_()
    Lo.image_loss(a, b, ssim_weight=1.0, pixel='charbonnier', crop_border=2, reduction='none').mul(_upstream(2).float().cuda()).sum().backward()
    assert a.grad is None and _grad_err(b.grad, _reference(shape, *view)[2]) <= GRAD_TOL
    assert not Lo.image_loss(a.detach(), b.detach(), ssim_weight=1.0).requires_grad


def test_two_calls_are_bit_equal():
    for view in ((0, False, 'charbonnier+ssim'), (4, True, 'ssim'), (2, False, 'l1')):
        first, second = _fused((1, 3, 96, 192), *view), _fused((1, 3, 96, 192), *view)
        assert all(torch.equal(x, y) for x, y in zip(first, second))


def test_non_contiguous_inputs_equal_their_contiguous_copies():
    Lo = pkg('losses')
    shape = (2, 3, 45, 70)
    a0, b0 = (t.cuda() for t in _images(shape))
    want = _fused(shape, 2, False, 'charbonnier+ssim')
    g = _upstream(2).float().cuda()
    cl = [t.contiguous(memory_format=torch.channels_last) for t in (a0, b0)]
    sl = [F.pad(t, (2, 3, 1, 1), value=0.5)[:, :, 1:-1, 2:-3] for t in (a0, b0)]
    for a, b in (cl, sl):
        assert not a.is_contiguous() and torch.equal(a, a0)
        a, b = a.detach().requires_grad_(), b.detach().requires_grad_()
        loss = Lo.image_loss(a, b, crop_border=2, reduction='none', **CONFIGS['charbonnier+ssim'])
        (loss * g).sum().backward()
        assert torch.equal(loss.detach(), want[0])
        assert a.grad.shape == shape and torch.equal(a.grad, want[1]) and torch.equal(b.grad, want[2])


def test_return_parts_and_reductions():
    """ssim is the metric's value bit for bit: the loss forward and the metric launch the same tile kernel (csrc/sisr_ssim.h)
    and fold its partials in the same order"""
    Lo, M = pkg('losses'), pkg('metrics')
    shape, crop, luma = (2, 3, 45, 70), 2, False
    a, b = (t.cuda() for t in _images(shape))
    kw = dict(ssim_weight=0.5, pixel_weight=2.0, pixel='charbonnier', crop_border=crop, luma=luma)
    loss, ssim, pix = Lo.image_loss(a, b, reduction='none', return_parts=True, **kw)
    a64, b64 = (t.double() for t in _images(shape))
    want, want_ssim, want_pix = _definition(a64, b64, **kw)
    for t in (loss, ssim, pix):
        assert t.shape == (2,) and t.dtype == torch.float32 and t.is_cuda and not t.requires_grad
    assert torch.equal(ssim, M.ssim(a, b, crop_border=crop, luma=luma))
    assert float((ssim.double().cpu() - want_ssim).abs().max()) <= FWD_TOL
    assert float((pix.double().cpu() - want_pix).abs().max()) <= FWD_TOL
    assert float((loss.double().cpu() - want).abs().max()) <= 2.5 * FWD_TOL          # 0.5 and 2.0 times the two terms' bounds
    assert torch.equal(Lo.image_loss(a, b, reduction='none', **kw), loss)
    mean = Lo.image_loss(a, b, **kw)
    assert mean.shape == () and torch.equal(mean, loss.mean())
    # the parts of a pixel-only loss: the SSIM is computed all the same
    _, ssim0, pix0 = Lo.image_loss(a, b, pixel='charbonnier', crop_border=crop, return_parts=True)
    assert torch.equal(ssim0, ssim) and torch.equal(pix0, pix)
    # the one-term wrappers
    assert torch.equal(Lo.ssim_loss(a, b, crop_border=crop), Lo.image_loss(a, b, ssim_weight=1.0, pixel_weight=0.0, crop_border=crop))
    assert torch.equal(Lo.l1_loss(a, b, luma=True), Lo.image_loss(a, b, pixel='l1', luma=True))
    assert torch.equal(Lo.charbonnier_loss(a, b, eps=1e-2), Lo.image_loss(a, b, pixel='charbonnier', eps=1e-2))


@pytest.mark.parametrize('shape,crop,luma', [(s, crop, luma) for s in SHAPES for crop, luma in VIEWS
                                             if min(s[2], s[3]) - 2 * crop >= WINDOW])
def test_mse_parts_are_the_metrics_values(shape, crop, luma):
    """pixel='mse' with return_parts runs the metric's own instantiation of the tile kernel: ssim equals metrics.ssim bit for
    bit, and pix is the mean squared difference under metrics.psnr.  Both come from the same double sum; rounding pix to fp32 moves
    the decibel value by at most 2.6e-7 dB and the fp32 psnr (below 64 dB) carries at most 1.9e-6 dB: 1e-5 dB leaves room for the
    log10 of this float64 evaluation and nothing else"""
    Lo, M = pkg('losses'), pkg('metrics')
    a, b = (t.cuda() for t in _images(shape))
    _, ssim, pix = Lo.image_loss(a, b, pixel='mse', crop_border=crop, luma=luma, reduction='none', return_parts=True)
    psnr, m_ssim = M.psnr_ssim(a, b, crop_border=crop, luma=luma)
    assert torch.equal(ssim, m_ssim) and torch.equal(ssim, M.ssim(a, b, crop_border=crop, luma=luma))
    e_psnr = float((psnr.double() - 10.0 * torch.log10(2.0 ** 2 / pix.double())).abs().max())
    print('image_loss mse parts %s crop %d luma %d: psnr - 10 log10(range^2 / pix) = %.3g dB' % (shape, crop, luma, e_psnr))
    assert e_psnr <= 1e-5


def test_launch_sequence_is_capturable_and_replays_on_new_contents():
    """no host synchronisation on the path: GraphedStep captures forward + backward (a GraphCaptureError fails the test) and a
    replay after new contents were copied into the static inputs equals an eager call on those contents"""
    Lo, G = pkg('losses'), pkg('graph')
    shape = (2, 3, 45, 70)
    a0, b0 = (t.cuda() for t in _images(shape))
    a1, b1 = (t.cuda() for t in _images(shape, seed=1))
    g = _upstream(2).float().cuda()

    def fwd_bwd(a, b):
        a, b = a.detach().requires_grad_(), b.detach().requires_grad_()
        loss = Lo.image_loss(a, b, ssim_weight=1.0, pixel='charbonnier', crop_border=2, luma=True, reduction='none')
        return (loss,) + torch.autograd.grad((loss * g).sum(), (a, b))
    sa, sb = a0.clone(), b0.clone()
    step = G.GraphedStep(lambda: fwd_bwd(sa, sb))
    out, eager0 = step(), fwd_bwd(a0, b0)
    assert all(torch.equal(x, y) for x, y in zip(out, eager0))
    sa.copy_(a1)
    sb.copy_(b1)
    out, eager1 = step(), fwd_bwd(a1, b1)
    assert not torch.equal(eager1[0], eager0[0])
    assert all(torch.equal(x, y) for x, y in zip(out, eager1))


def test_one_generator_step_matches_the_torch_composition_of_the_loss():
    """Generator(1, 16, 64, [2]) on a (2, 3, 16, 16) LR batch: the parameter gradients through the fused loss against those through
    the same net output and the gradient of the loss's torch-op composition (float64 on the CPU), within the project's 1e-3"""
    Lo = pkg('losses')
    torch.manual_seed(11)
    net = pkg('model_generator').Generator(1, 16, 64, [2]).cuda().train()
    state = {k: v.detach().clone() for k, v in net.state_dict().items()}
    gen = torch.Generator().manual_seed(12)
    lr = (torch.rand(2, 3, 16, 16, generator=gen) * 2 - 1).cuda()
    hr = (torch.rand(2, 3, 32, 32, generator=gen) * 2 - 1).cuda()
    kw = dict(ssim_weight=0.5, pixel_weight=1, pixel='charbonnier')
    out = net(lr)
    assert out.shape == hr.shape
    loss = Lo.image_loss(out, hr, **kw)
    loss.backward()
    got = {k: p.grad.detach().cpu().clone() for k, p in net.named_parameters()}
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    # the composition on the same net output
    out64 = out.detach().double().cpu().requires_grad_()
    want = _definition(out64, hr.double().cpu(), **kw)[0].mean()
    d_out, = torch.autograd.grad(want, out64)
    assert abs(float(loss) - float(want)) <= 2 * FWD_TOL
    net.load_state_dict(state)
    net.zero_grad(set_to_none=True)
    out2 = net(lr)
    assert torch.equal(out2, out)
    out2.backward(d_out.float().cuda())
    ref = {k: p.grad.detach().cpu() for k, p in net.named_parameters()}
    assert grads_close(got, ref, 1e-3) == []
