"""GPU: metrics.psnr / ssim / psnr_ssim / evaluate_generator (csrc/metrics.hip) against the definition evaluated in float64 on
the CPU: crop and luma view, separable 11-tap Gaussian (sigma 1.5) through F.conv2d, "valid" positions, plain means.

Inputs are structured (a smooth pattern per image and plane, plus noise whose strength grows along x), so that an indexing mistake
moves the result: one pixel of error in the valid region or in the crop changes SSIM by >= 1.3e-4 and PSNR by >= 2.8e-3 dB on this
recipe, while evaluating the formula in fp32 instead of fp64 changes them by <= 1.4e-7 and <= 2.2e-6 dB.  The bounds sit between:
SSIM 2e-5 absolute, PSNR 1e-3 dB absolute.

The kernel's tile is 16 x 32 window positions: (1, 3, 96, 192) has 86 x 182 of them = 6 x 6 tiles with ragged last ones in both
axes, (2, 3, 45, 70) and (3, 3, 64, 64) give ragged 3 x 2 / 4 x 2 grids, (1, 1, 11, 11) is a single window position and
(2, 3, 13, 17) a 3 x 7 region inside one tile."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from gpu_helpers import pkg
from image_cases import _definition, _images

pytestmark = pytest.mark.gpu

SSIM_TOL = 2e-5
PSNR_TOL = 1e-3

SHAPES = [(1, 1, 11, 11), (2, 3, 13, 17), (2, 3, 45, 70), (3, 3, 64, 64), (1, 3, 96, 192)]
VIEWS = [(0, False), (2, False), (4, True)]
VALUE_CASES = [(s, crop, luma) for s in SHAPES for crop, luma in VIEWS if min(s[2], s[3]) - 2 * crop >= 11]


def _reference(a, b, data_range, crop, luma):
    """-> (psnr [N], ssim [N]) in float64: the shared definition with the squared difference as its pixel term"""
    _, ssim, mse = _definition(a.double(), b.double(), pixel='mse', data_range=data_range, crop_border=crop, luma=luma)
    return 10.0 * torch.log10(data_range ** 2 / mse), ssim


@functools.lru_cache(maxsize=None)
def _reference_of(shape, crop, luma):
    a, b = _images(shape)
    return _reference(a, b, 2.0, crop, luma)


def _err(got, want):
    return float((got.double().cpu() - want).abs().max())


@pytest.mark.parametrize('shape,crop,luma', VALUE_CASES)
def test_values_match_the_float64_definition(shape, crop, luma):
    M = pkg('metrics')
    a, b = (t.cuda() for t in _images(shape))
    rp, rs = _reference_of(shape, crop, luma)
    p = M.psnr(a, b, crop_border=crop, luma=luma)
    s = M.ssim(a, b, crop_border=crop, luma=luma)
    p2, s2 = M.psnr_ssim(a, b, crop_border=crop, luma=luma)
    for t in (p, s, p2, s2):
        assert t.shape == (shape[0],) and t.dtype == torch.float32 and t.device == a.device
    errs = _err(p, rp), _err(p2, rp), _err(s, rs), _err(s2, rs)
    print('metrics %s crop %d luma %d: psnr err %.3g / %.3g dB, ssim err %.3g / %.3g' % ((shape, crop, luma) + errs))
    assert max(errs[:2]) <= PSNR_TOL and max(errs[2:]) <= SSIM_TOL, errs


def test_identical_images_give_infinite_psnr_and_unit_ssim():
    M = pkg('metrics')
    a = _images((2, 3, 45, 70))[0].cuda()
    p, s = M.psnr_ssim(a, a.clone(), crop_border=1)
    assert torch.all(torch.isposinf(p)), p
    assert float((s - 1).abs().max()) <= 1e-6, s
    assert torch.all(torch.isposinf(M.psnr(a, a)))


def test_scaling_images_and_data_range_together_changes_nothing():
    M = pkg('metrics')
    shape, crop = (2, 3, 45, 70), 2
    a, b = (t.cuda() for t in _images(shape))
    rp, rs = _reference_of(shape, crop, False)
    p1, s1 = M.psnr_ssim(a, b, crop_border=crop)
    p255, s255 = M.psnr_ssim(127.5 * a, 127.5 * b, data_range=255, crop_border=crop)
    print('metrics scaled by 127.5: psnr %.3g dB, ssim %.3g from the unscaled call; %.3g dB, %.3g from the reference'
          % (_err(p255, p1.double().cpu()), _err(s255, s1.double().cpu()), _err(p255, rp), _err(s255, rs)))
    assert _err(p255, p1.double().cpu()) <= PSNR_TOL and _err(s255, s1.double().cpu()) <= SSIM_TOL
    assert _err(p255, rp) <= PSNR_TOL and _err(s255, rs) <= SSIM_TOL


def test_two_calls_are_bit_equal():
    M = pkg('metrics')
    a, b = (t.cuda() for t in _images((1, 3, 96, 192)))
    p1, s1 = M.psnr_ssim(a, b, crop_border=4, luma=True)
    p2, s2 = M.psnr_ssim(a, b, crop_border=4, luma=True)
    assert torch.equal(p1, p2) and torch.equal(s1, s2)
    assert torch.equal(M.psnr(a, b, crop_border=4, luma=True), p1) and torch.equal(M.ssim(a, b, crop_border=4, luma=True), s1)


def test_non_contiguous_inputs_equal_their_contiguous_copies():
    M = pkg('metrics')
    a, b = (t.cuda() for t in _images((2, 3, 45, 70)))
    want = M.psnr_ssim(a, b, crop_border=2)
    cl_a, cl_b = a.contiguous(memory_format=torch.channels_last), b.contiguous(memory_format=torch.channels_last)
    assert not cl_a.is_contiguous()
    got = M.psnr_ssim(cl_a, cl_b, crop_border=2)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    big_a, big_b = (F.pad(t, (2, 3, 1, 1), value=0.5) for t in (a, b))
    sl_a, sl_b = big_a[:, :, 1:-1, 2:-3], big_b[:, :, 1:-1, 2:-3]
    assert not sl_a.is_contiguous() and torch.equal(sl_a, a)
    got = M.psnr_ssim(sl_a, sl_b, crop_border=2)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_launch_sequence_is_capturable_and_replays_on_new_contents():
    """no host synchronisation on the path: GraphedStep captures it (a GraphCaptureError fails the test) and a replay after new
    contents were copied into the static inputs equals an eager call on those contents"""
    M, G = pkg('metrics'), pkg('graph')
    shape = (2, 3, 45, 70)
    a0, b0 = (t.cuda() for t in _images(shape))
    a1, b1 = (t.cuda() for t in _images(shape, seed=1))
    sa, sb = a0.clone(), b0.clone()
    step = G.GraphedStep(lambda: M.psnr_ssim(sa, sb, crop_border=2, luma=True))
    p, s = step()
    e = M.psnr_ssim(a0, b0, crop_border=2, luma=True)
    assert torch.equal(p, e[0]) and torch.equal(s, e[1])
    sa.copy_(a1)
    sb.copy_(b1)
    p, s = step()
    e = M.psnr_ssim(a1, b1, crop_border=2, luma=True)
    assert not torch.equal(e[1], M.ssim(a0, b0, crop_border=2, luma=True))
    assert torch.equal(p, e[0]) and torch.equal(s, e[1])


def _generator_and_batch():
    torch.manual_seed(5)
    net = pkg('model_generator').Generator(1, 16, 64, [2], use_sn=True).cuda().train()
    hr = (torch.rand(2, 3, 32, 32, generator=torch.Generator().manual_seed(6)) * 2 - 1).cuda()
    return net, hr


def test_evaluate_generator_equals_the_manual_pipeline_and_leaves_the_net_untouched():
    M, ut = pkg('metrics'), pkg('utils')
    net, hr = _generator_and_batch()
    before = {k: v.clone() for k, v in net.state_dict().items()}
    assert any('running_mean' in k for k in before) and any('num_batches_tracked' in k for k in before)
    assert any(k.endswith('_u') for k in before) and any(k.endswith('_v') for k in before)
    out = M.evaluate_generator(net, hr, (16, 16))
    assert net.training and all(m.training for m in net.modules())
    after = net.state_dict()
    assert list(after.keys()) == list(before.keys())
    changed = [k for k in before if not torch.equal(before[k], after[k])]
    assert not changed, changed
    net.eval()
    with torch.no_grad():
        sr = net(ut.lr_from_hr(hr, (16, 16)))
    p, s = M.psnr_ssim(sr, hr, crop_border=2)
    assert sorted(out) == ['psnr', 'ssim']
    assert torch.equal(out['psnr'], p) and torch.equal(out['ssim'], s)
    assert bool(torch.isfinite(p).all()) and bool(((s > -1) & (s < 1)).all())


def test_evaluate_generator_refuses_an_hr_batch_of_the_wrong_size():
    M = pkg('metrics')
    net, _ = _generator_and_batch()
    hr = torch.zeros(2, 3, 40, 40, device='cuda')
    with pytest.raises(ValueError):
        M.evaluate_generator(net, hr, (16, 16))
    assert net.training
