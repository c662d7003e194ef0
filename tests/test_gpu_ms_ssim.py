"""GPU: metrics.ms_ssim and losses.ms_ssim_loss (csrc/ms_ssim.hip), forward and backward, against the definition of
ms_ssim_cases.py evaluated in float64 on the CPU from the same fp32 inputs, with the gradients from torch autograd.

Inputs: image_cases._images (a smooth pattern per image and plane plus noise whose strength grows along x, never constant).  The
value cases (ms_ssim_cases.VALUE_CASES) are each the smallest shape at which one thing can go wrong: one window position without a
pyramid; a level that is exactly 11 x 11 with a dropped odd column; ragged tiles with pooled seams at the 16th / 32nd pixel, an odd
height and a crop that shifts the cell parity; luma with crop and odd sizes; 6 x 6 tiles with two and three pooled levels; five
levels ending in one window position; five levels with odd sizes, plain and under crop + luma.  The upstream gradient differs from
image to image (reduction='none', (loss * g).sum()).

Bounds, the project's own: |loss - ref| <= 2e-5, |terms - ref| <= 2e-5, max|grad - ref| <= 1e-4 max|ref| for da and for db.
Evaluating the same formula in fp32 instead of fp64 on the CPU moves, over these cases, the loss by at most 1.6e-7, the terms by at
most 4.8e-7 and the gradients by at most 6.7e-6 of max|ref| (db at (1, 1, 176, 176)): test_ms_ssim_cpu.py asserts a tenth of each
bound.  Every term of these cases is 0.258 or more, so the t <= 0 rule is not in play in the value test; it has a test of its own.

Loss against metric: the loss is the fp32 difference 1 - ms_ssim, so `loss == 1 - ms_ssim` holds bit for bit always; `1 - loss ==
ms_ssim` holds bit for bit exactly when ms_ssim >= 0.5 (both differences are then exact in fp32, Sterbenz), and below 0.5 the loss
carries fewer bits than the score: there 1 - loss (exact again) is within the rounding of the loss, 2^-25, of it.  The test
asserts all three."""
import pytest
import torch
import torch.nn.functional as F

from gpu_helpers import pkg
from helpers import grads_close
from image_cases import _images
from ms_ssim_cases import MS_SSIM_WEIGHTS, VALUE_CASES, _ms_definition, _reference, _upstream

pytestmark = pytest.mark.gpu

FWD_TOL = 2e-5
GRAD_TOL = 1e-4
W2 = MS_SSIM_WEIGHTS[:2]


def _fused(shape, weights, crop, luma, seed=0, want_a=True, want_b=True):
    """forward + backward on the device -> (loss [N], da or None, db or None)"""
    Lo = pkg('losses')
    a, b = (t.cuda() for t in _images(shape, seed))
    a.requires_grad_(want_a)
    b.requires_grad_(want_b)
    loss = Lo.ms_ssim_loss(a, b, crop_border=crop, luma=luma, weights=weights, reduction='none')
    (loss * _upstream(shape[0]).float().cuda()).sum().backward()
    return loss.detach(), a.grad, b.grad


def _grad_err(got, want):
    return float((got.double().cpu() - want).abs().max() / want.abs().max())


@pytest.mark.parametrize('shape,weights,crop,luma', VALUE_CASES)
def test_loss_terms_and_gradients_match_the_float64_definition(shape, weights, crop, luma):
    want, want_terms, want_da, want_db = _reference(shape, weights, crop, luma)
    loss, da, db = _fused(shape, weights, crop, luma)
    a, b = (t.cuda() for t in _images(shape))
    ms, terms = pkg('metrics').ms_ssim(a, b, crop_border=crop, luma=luma, weights=weights, return_terms=True)
    assert loss.shape == (shape[0],) and loss.dtype == torch.float32 and loss.is_cuda
    assert ms.shape == (shape[0],) and ms.dtype == torch.float32 and ms.is_cuda and not ms.requires_grad
    assert terms.shape == want_terms.shape and terms.dtype == torch.float32 and terms.is_cuda
    assert da.shape == shape and db.shape == shape
    e_fwd = float((loss.double().cpu() - want).abs().max())
    e_ms = float(((1 - ms.double().cpu()) - want).abs().max())
    e_terms = float((terms.double().cpu() - want_terms).abs().max())
    e_a, e_b = _grad_err(da, want_da), _grad_err(db, want_db)
    print('ms_ssim %s M %d crop %d luma %d: loss err %.3g, metric err %.3g, terms err %.3g, da err %.3g, db err %.3g of max|ref|'
          % (shape, len(weights), crop, luma, e_fwd, e_ms, e_terms, e_a, e_b))
    assert e_fwd <= FWD_TOL and e_ms <= FWD_TOL
    assert e_terms <= FWD_TOL
    assert e_a <= GRAD_TOL and e_b <= GRAD_TOL


@pytest.mark.parametrize('shape,crop,luma', [((2, 3, 45, 70), 2, False), ((1, 3, 96, 192), 4, True)])
def test_one_scale_of_weight_one_is_the_ssim_metric(shape, crop, luma):
    """the same window and tile grid, a fold per plane in place of a fold per image: equal up to the order of summation"""
    M = pkg('metrics')
    a, b = (t.cuda() for t in _images(shape))
    ms = M.ms_ssim(a, b, crop_border=crop, luma=luma, weights=(1.0,))
    ssim = M.ssim(a, b, crop_border=crop, luma=luma)
    print('ms_ssim one scale %s: |ms_ssim - ssim| = %.3g' % (shape, float((ms - ssim).abs().max())))
    assert float((ms.double() - ssim.double()).abs().max()) <= 1e-6


@pytest.mark.parametrize('shape,crop,luma', [((1, 1, 11, 11), 0, False), ((2, 3, 45, 70), 2, False), ((1, 3, 37, 50), 1, True)])
def test_one_scale_of_weight_one_has_the_ssim_loss_gradient_bit_for_bit(shape, crop, luma):
    """one window position; ragged tiles on both axes with three planes; the three-channel store under luma.  The two backward
    kernels run the same text (csrc/sisr_ssim_bwd.h, contraction off) on the same map; with upstream ones the image loss adds a
    pixel term of exactly 0 and MS-SSIM no pooled gradient, and the two factors in front of the window gradient,
    (float)(-(1 / C') (1 / (Hv Wv))) times pow(t, 1) / t and (float)(-1 / (C' Hv Wv)), are the same float for these shapes
    (every term of these cases is 0.29 or more: the t <= 0 rule is not in play)"""
    Lo = pkg('losses')
    kw = dict(crop_border=crop, luma=luma, reduction='none')
    for want_b in (True, False):
        grads = []
        for loss_of in (lambda a, b: Lo.ms_ssim_loss(a, b, weights=(1.0,), **kw), lambda a, b: Lo.ssim_loss(a, b, **kw)):
            a, b = (t.cuda() for t in _images(shape))
            a.requires_grad_()
            b.requires_grad_(want_b)
            loss_of(a, b).sum().backward()
            grads.append((a.grad, b.grad))
        (ms_da, ms_db), (il_da, il_db) = grads
        assert ms_da.shape == shape and bool((ms_da != 0).any())
        assert torch.equal(ms_da, il_da)
        if want_b:
            assert torch.equal(ms_db, il_db)
        else:
            assert ms_db is None and il_db is None


@pytest.mark.parametrize('shape,weights,crop,luma', [VALUE_CASES[2], VALUE_CASES[4], VALUE_CASES[6]])
def test_loss_is_one_minus_the_metric(shape, weights, crop, luma):
    Lo, M = pkg('losses'), pkg('metrics')
    a, b = (t.cuda() for t in _images(shape))
    kw = dict(crop_border=crop, luma=luma, weights=weights)
    loss, ms = Lo.ms_ssim_loss(a, b, reduction='none', **kw), M.ms_ssim(a, b, **kw)
    assert torch.equal(loss, 1 - ms)
    back = 1 - loss
    high = ms >= 0.5
    assert torch.equal(back[high], ms[high])
    assert float((back.double() - ms.double()).abs().max()) <= 2.0 ** -25
    mean = Lo.ms_ssim_loss(a, b, **kw)
    assert mean.shape == () and torch.equal(mean, loss.mean())


def _dirty(shape):
    dirty = [torch.full(shape, float('nan'), device='cuda') for _ in range(2)]
    del dirty                                    # two free blocks of the gradients' size, full of NaNs


def test_a_term_that_is_not_positive_gives_zero_and_zero_gradients():
    """b = -a with a the noisy image of the pair: the first scale's structure term is negative in every plane (-0.73, -0.79, -0.81 in
    the float64 definition), a fractional power of it would be a NaN: the score is exactly 0 and so is every gradient.  The
    gradients are torch.empty: blocks that held NaNs are handed back to the backward, which must write every element.
    With a the smooth image of the pair the rule is per (image, plane): plane 0 keeps positive terms (0.24, 0.23) and its value
    and gradient, planes 1 and 2 (-0.06, -0.32 at the first scale) get exact zeros"""
    Lo, M = pkg('losses'), pkg('metrics')
    shape = (1, 3, 45, 70)
    a0 = _images(shape)[1]
    ref_ms, ref_terms = _ms_definition(a0.double(), -a0.double(), W2)
    assert bool((ref_terms <= 0).any(dim=0).all()) and float(ref_terms.min()) < -0.8 and float(ref_ms) == 0.0
    a, b = a0.cuda().requires_grad_(), (-a0).cuda().requires_grad_()
    ms, terms = M.ms_ssim(a, b, weights=W2, return_terms=True)
    assert float((terms.double().cpu() - ref_terms).abs().max()) <= FWD_TOL
    assert bool((ms == 0).all())
    loss = Lo.ms_ssim_loss(a, b, weights=W2, reduction='none')
    assert bool((loss == 1).all())
    _dirty(shape)
    loss.sum().backward()
    for grad in (a.grad, b.grad):
        assert bool(torch.isfinite(grad).all()) and bool((grad == 0).all())
    # per plane
    a0 = _images(shape)[0]
    a64, b64 = a0.double().requires_grad_(), (-a0.double()).requires_grad_()
    ref_ms, ref_terms = _ms_definition(a64, b64, W2)
    assert (ref_terms > 0).all(dim=0).tolist() == [[True, False, False]]
    want = torch.autograd.grad((1 - ref_ms).sum(), (a64, b64))
    a, b = a0.cuda().requires_grad_(), (-a0).cuda().requires_grad_()
    loss = Lo.ms_ssim_loss(a, b, weights=W2, reduction='none')
    assert abs(float(loss.detach()) - float(1 - ref_ms.detach())) <= FWD_TOL
    _dirty(shape)
    loss.sum().backward()
    for grad, ref in zip((a.grad, b.grad), want):
        assert bool(torch.isfinite(grad).all()) and bool((grad[:, 1:] == 0).all()) and bool((ref[:, 1:] == 0).all())
        assert _grad_err(grad, ref) <= GRAD_TOL


@pytest.mark.parametrize('shape,weights', [((2, 3, 45, 70), W2), ((1, 1, 11, 11), (1.0,))])
def test_equal_images_give_zero_loss_and_a_vanishing_gradient(shape, weights):
    Lo = pkg('losses')
    a = _images(shape)[0].cuda().requires_grad_()
    b = a.detach().clone()
    loss = Lo.ms_ssim_loss(a, b, weights=weights, reduction='none')
    (loss * _upstream(shape[0]).float().cuda()).sum().backward()
    scale = float(_reference(shape, weights, 0, False)[2].abs().max())        # the unequal pair of the same shape
    print('ms_ssim equal images %s: loss %.3g, max|da| %.3g of the unequal pair\'s' % (shape, float(loss.abs().max()), float(a.grad.abs().max()) / scale))
    assert float(loss.abs().max()) <= 1e-6
    assert float(a.grad.abs().max()) <= 1e-4 * scale


def test_cropped_border_gets_exact_zeros_from_a_dirty_allocator():
    Lo = pkg('losses')
    shape, crop = (2, 3, 47, 71), 2
    for luma in (False, True):
        a, b = (t.cuda().requires_grad_() for t in _images(shape))
        loss = Lo.ms_ssim_loss(a, b, crop_border=crop, luma=luma, weights=W2)
        _dirty(shape)
        loss.backward()
        for grad in (a.grad, b.grad):
            assert bool(torch.isfinite(grad).all())
            inner = torch.zeros(shape, dtype=torch.bool, device='cuda')
            inner[:, :, crop:shape[2] - crop, crop:shape[3] - crop] = True
            assert bool((grad[~inner] == 0).all())
            assert bool((grad[inner] != 0).any())


def test_luma_gradients_are_the_luma_gradient_times_the_coefficients():
    shape, crop = (2, 3, 47, 71), 2
    _, da, db = _fused(shape, W2, crop, True)
    for grad in (da, db):
        g = grad.double().cpu()
        nz = g[:, 0] != 0
        assert not bool(nz[:, :2].any()) and not bool(nz[:, :, :2].any())          # the cropped border
        assert int(nz.sum()) >= 0.99 * 2 * 43 * 67                                 # the view (43 x 67 per image)
        assert float((g[:, 1][nz] / g[:, 0][nz] - 0.587 / 0.299).abs().max()) <= 1e-6
        assert float((g[:, 2][nz] / g[:, 0][nz] - 0.114 / 0.299).abs().max()) <= 1e-6


def test_only_the_gradient_asked_for_is_computed():
    for shape, weights, crop, luma in (VALUE_CASES[3], VALUE_CASES[6], VALUE_CASES[0]):
        loss2, da2, db2 = _fused(shape, weights, crop, luma)
        loss1, da1, db1 = _fused(shape, weights, crop, luma, want_b=False)
        assert db1 is None and torch.equal(da1, da2) and torch.equal(loss1, loss2)
        loss0, da0, db0 = _fused(shape, weights, crop, luma, want_a=False)
        assert da0 is None and torch.equal(db0, db2) and torch.equal(loss0, loss2)
    Lo = pkg('losses')
    a, b = (t.cuda() for t in _images((2, 3, 45, 70)))
    assert not Lo.ms_ssim_loss(a, b, weights=W2).requires_grad


def test_two_calls_are_bit_equal():
    for case in (VALUE_CASES[3], VALUE_CASES[6]):
        first, second = _fused(*case), _fused(*case)
        assert all(torch.equal(x, y) for x, y in zip(first, second))


def test_non_contiguous_inputs_equal_their_contiguous_copies():
    Lo = pkg('losses')
    shape = (2, 3, 45, 70)
    a0, b0 = (t.cuda() for t in _images(shape))
    want = _fused(shape, W2, 1, False)
    g = _upstream(2).float().cuda()
    cl = [t.contiguous(memory_format=torch.channels_last) for t in (a0, b0)]
    sl = [F.pad(t, (2, 3, 1, 1), value=0.5)[:, :, 1:-1, 2:-3] for t in (a0, b0)]
    for a, b in (cl, sl):
        assert not a.is_contiguous() and torch.equal(a, a0)
        a, b = a.detach().requires_grad_(), b.detach().requires_grad_()
        loss = Lo.ms_ssim_loss(a, b, crop_border=1, weights=W2, reduction='none')
        (loss * g).sum().backward()
        assert torch.equal(loss.detach(), want[0])
        assert a.grad.shape == shape and torch.equal(a.grad, want[1]) and torch.equal(b.grad, want[2])


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
        loss = Lo.ms_ssim_loss(a, b, crop_border=1, luma=True, weights=W2, reduction='none')
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
    """Generator(1, 16, 64, [2]) on a (2, 3, 16, 16) LR batch (HR 32 x 32, two scales): the parameter gradients through the fused
    loss against those through the same net output and the gradient of the float64 composition, within the project's 1e-3"""
    Lo = pkg('losses')
    torch.manual_seed(11)
    net = pkg('model_generator').Generator(1, 16, 64, [2]).cuda().train()
    state = {k: v.detach().clone() for k, v in net.state_dict().items()}
    gen = torch.Generator().manual_seed(12)
    lr = (torch.rand(2, 3, 16, 16, generator=gen) * 2 - 1).cuda()
    out = net(lr)
    assert out.shape == (2, 3, 32, 32)
    # an HR batch that resembles the output (the output plus noise), so that every term is positive and a gradient flows
    hr = (out.detach().cpu() + 0.2 * torch.randn(2, 3, 32, 32, generator=gen)).clamp(-1, 1).cuda()
    loss = Lo.ms_ssim_loss(out, hr, weights=W2)
    loss.backward()
    got = {k: p.grad.detach().cpu().clone() for k, p in net.named_parameters()}
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    # the composition on the same net output
    out64 = out.detach().double().cpu().requires_grad_()
    ref_ms, ref_terms = _ms_definition(out64, hr.double().cpu(), W2)
    assert float(ref_terms.min()) > 0
    want = (1 - ref_ms).mean()
    d_out, = torch.autograd.grad(want, out64)
    assert abs(float(loss) - float(want)) <= FWD_TOL
    net.load_state_dict(state)
    net.zero_grad(set_to_none=True)
    out2 = net(lr)
    assert torch.equal(out2, out)
    out2.backward(d_out.float().cuda())
    ref = {k: p.grad.detach().cpu() for k, p in net.named_parameters()}
    assert grads_close(got, ref, 1e-3) == []
