"""CPU: the host side of the frequency-domain loss (losses.frequency_loss, csrc/freq_loss.hip) and the conditions its GPU tests
stand on:

  * the closed form the kernels evaluate for the focal loss (half spectrum, Hermitian weights) equals the literal formulation
    (full fft2, norm='ortho', weight matrix) in float64, with W' even and odd;
  * a == b gives 0 and a zero gradient in the definition;
  * argument validation: ValueError BEFORE the device is looked at, RuntimeError for CPU tensors (no fallback);
  * the workspace query of the C ABI;
  * the L1 sign margin condition on every case whose L1 gradient the GPU test compares: the smallest |Re D| or |Im D| that is not
    structurally zero is at least 1e-4 max|D| in the float64 reference.  A condition on the inputs, not a tolerance: one flipped
    sign moves the whole gradient by about 2 / sqrt(count), and the minimum over thousands of bins shrinks as 1 / count, so the
    larger cases compare the L1 value only;
  * the error of the definition evaluated in fp32 against float64, per case: the floor under the GPU bounds (2e-5 |ref| for the
    loss, 1e-4 max|ref| for the gradients).  Measured: loss <= 2.8e-7 relative; gradient <= 9.7e-6 of max|ref| (worst:
    charbonnier at 192 x 192), <= 4.7e-7 for l1 and focal."""
import importlib

import pytest
import torch

from freq_cases import CASES, KINDS, L1_GRAD_CASES, SIGN_MARGIN, _reference, closed_form_focal, defn, evaluate, structural_imag_zero
from image_cases import _images

E_BADARG, E_UNSUPPORTED = -1, -3


def _pkg(sub):
    return importlib.import_module('single-image-super-resolution_amd.' + sub)


def _ws(*args):
    return _pkg('_lib').lib().sisr_freq_loss_ws_floats(*args)


@pytest.mark.parametrize('shape,crop,luma', [((2, 3, 8, 9), 0, False), ((2, 3, 9, 8), 0, False), ((2, 3, 7, 9), 0, False),
                                             ((2, 1, 4, 6), 0, False), ((2, 3, 21, 36), 2, True), ((1, 1, 1, 1), 0, False)])
@pytest.mark.parametrize('alpha', [1.0, 0.5, 3.0])
def test_closed_form_of_the_focal_loss_equals_the_literal_formulation(shape, crop, luma, alpha):
    a, b = (t.double() for t in _images(shape))
    want = defn(a, b, 'focal', crop, luma, alpha)[0]
    got = closed_form_focal(a, b, crop, luma, alpha)
    assert float(((got - want).abs() / want.abs()).max()) <= 1e-12


@pytest.mark.parametrize('kind', KINDS)
def test_equal_images_give_zero_and_a_zero_gradient_in_the_definition(kind):
    a = _images((2, 3, 8, 9))[0].double().requires_grad_()
    b = a.detach().clone().requires_grad_()
    loss = defn(a, b, kind, eps=0.0 if kind == 'charbonnier' else 1e-3)[0]
    if kind == 'charbonnier':              # sqrt(z^2 + 0) at 0: the value is 0, the derivative is not defined; with eps it is eps
        assert float(loss.detach().abs().max()) == 0.0
        return
    da, db = torch.autograd.grad(loss.sum(), (a, b))
    assert float(loss.detach().abs().max()) == 0.0
    assert float(da.abs().max()) == 0.0 and float(db.abs().max()) == 0.0
    assert float(closed_form_focal(a.detach(), b.detach()).abs().max()) == 0.0


def _t(*shape, dtype=torch.float32):
    return torch.full(shape, 0.5, dtype=dtype)


BAD = {
    'shape mismatch': lambda f: f(_t(2, 3, 16, 16), _t(2, 3, 16, 17)),
    '3-D input': lambda f: f(_t(3, 16, 16), _t(3, 16, 16)),
    'two channels': lambda f: f(_t(2, 2, 16, 16), _t(2, 2, 16, 16)),
    'float64': lambda f: f(_t(2, 3, 16, 16, dtype=torch.float64), _t(2, 3, 16, 16, dtype=torch.float64)),
    'bf16': lambda f: f(_t(2, 3, 16, 16, dtype=torch.bfloat16), _t(2, 3, 16, 16, dtype=torch.bfloat16)),
    'empty batch': lambda f: f(_t(0, 3, 16, 16), _t(0, 3, 16, 16)),
    'unknown kind': lambda f: f(_t(2, 3, 16, 16), _t(2, 3, 16, 16), kind='amplitude'),
    'unknown reduction': lambda f: f(_t(2, 3, 16, 16), _t(2, 3, 16, 16), reduction='sum'),
    'negative eps': lambda f: f(_t(2, 3, 16, 16), _t(2, 3, 16, 16), kind='charbonnier', eps=-1e-3),
    'nan eps': lambda f: f(_t(2, 3, 16, 16), _t(2, 3, 16, 16), kind='charbonnier', eps=float('nan')),
    'alpha zero': lambda f: f(_t(2, 3, 16, 16), _t(2, 3, 16, 16), kind='focal', alpha=0.0),
    'alpha negative': lambda f: f(_t(2, 3, 16, 16), _t(2, 3, 16, 16), kind='focal', alpha=-1.0),
    'alpha above 4': lambda f: f(_t(2, 3, 16, 16), _t(2, 3, 16, 16), kind='focal', alpha=4.5),
    'alpha nan': lambda f: f(_t(2, 3, 16, 16), _t(2, 3, 16, 16), alpha=float('nan')),
    'negative crop_border': lambda f: f(_t(2, 3, 16, 16), _t(2, 3, 16, 16), crop_border=-1),
    'fractional crop_border': lambda f: f(_t(2, 3, 16, 16), _t(2, 3, 16, 16), crop_border=1.5),
    'nothing left after the crop': lambda f: f(_t(2, 3, 16, 16), _t(2, 3, 16, 16), crop_border=8),
    'width 257': lambda f: f(_t(1, 1, 4, 257), _t(1, 1, 4, 257)),
    'height 257': lambda f: f(_t(1, 1, 257, 4), _t(1, 1, 257, 4)),
    'view 257 after the crop': lambda f: f(_t(1, 1, 259, 8), _t(1, 1, 259, 8), crop_border=1),
    'not a tensor': lambda f: f([0.5], _t(1, 1, 16, 16)),
}


@pytest.mark.parametrize('case', sorted(BAD))
def test_frequency_loss_bad_arguments_raise_value_error_before_the_device_check(case):
    with pytest.raises(ValueError):
        BAD[case](_pkg('losses').frequency_loss)


def test_wrappers_validate_like_frequency_loss():
    Lo = _pkg('losses')
    for f in (Lo.fft_l1_loss, Lo.focal_frequency_loss):
        with pytest.raises(ValueError):
            f(_t(2, 2, 16, 16), _t(2, 2, 16, 16))
        with pytest.raises(ValueError):
            f(_t(1, 1, 4, 257), _t(1, 1, 4, 257))
        with pytest.raises(ValueError):
            f(_t(2, 3, 16, 16), _t(2, 3, 16, 16), reduction='sum')
    with pytest.raises(ValueError):
        Lo.focal_frequency_loss(_t(2, 3, 16, 16), _t(2, 3, 16, 16), alpha=0.0)


def test_valid_cpu_tensors_are_refused():
    Lo = _pkg('losses')
    a, b = _t(2, 3, 16, 16), _t(2, 3, 16, 16)
    for call in (lambda: Lo.frequency_loss(a, b), lambda: Lo.frequency_loss(a, b, kind='charbonnier', reduction='none'),
                 lambda: Lo.frequency_loss(a, b, kind='focal', alpha=4.0, crop_border=2, luma=True),
                 lambda: Lo.frequency_loss(_t(1, 1, 258, 256), _t(1, 1, 258, 256), crop_border=1),      # a 256 x 254 view is legal
                 lambda: Lo.fft_l1_loss(a, b), lambda: Lo.focal_frequency_loss(a, b)):
        with pytest.raises(RuntimeError):
            call()


def test_workspace_query():
    """which 0: the row spectra + one (sum, max) pair per 8-column block of the column pass; 1 and 3: the spectrum
    [N][C'][H'][Wh][2]; 2: the plane maxima"""
    spec = 2 * 3 * 45 * 36 * 2
    assert _ws(2, 3, 45, 70, 0, 0, 1) == spec and _ws(2, 3, 45, 70, 0, 0, 3) == spec
    assert _ws(2, 3, 45, 70, 0, 0, 0) == spec + 2 * 2 * 3 * 5                # Wh = 36: five blocks of 8 columns
    assert _ws(2, 3, 45, 70, 0, 0, 2) == 6 and _ws(2, 3, 45, 70, 0, 1, 2) == 2
    assert _ws(1, 3, 96, 96, 4, 1, 1) == 88 * 45 * 2                          # crop 4 + luma: one plane of 88 x 88
    assert _ws(1, 1, 1, 1, 0, 0, 0) == 2 + 2
    assert _ws(1, 1, 256, 256, 0, 0, 1) > 0 and _ws(1, 3, 258, 260, 2, 0, 1) > 0 and _ws(1, 1, 258, 258, 1, 0, 0) > 0
    for which in range(4):
        assert _ws(1, 1, 257, 16, 0, 0, which) < 0 and _ws(1, 1, 16, 257, 0, 0, which) < 0       # a side above 256
        assert _ws(1, 3, 260, 64, 1, 0, which) < 0                                             # 258 left after the crop
        assert _ws(2, 2, 45, 70, 0, 0, which) == E_UNSUPPORTED                                 # C = 2
        assert _ws(0, 3, 45, 70, 0, 0, which) == E_BADARG
        assert _ws(2, 3, 45, 70, 23, 0, which) == E_BADARG                                     # nothing left
        assert _ws(2, 3, 45, 70, -1, 0, which) == E_BADARG
    assert _ws(2, 3, 45, 70, 0, 0, 4) == E_BADARG and _ws(2, 3, 45, 70, 0, 0, -1) == E_BADARG


def test_entry_points_refuse_bad_scalars_before_any_launch():
    """a negative eps, alpha outside (0, 4], an unknown kind and a side above 256 are refused (the pointers are never used)"""
    lib, one = _pkg('_lib').lib(), 1
    shape = (2, 3, 45, 70, 0, 0)

    def fwd(kind=0, eps=1e-3, alpha=1.0, shape=shape):
        return lib.sisr_freq_loss_fwd(one, one, *shape, kind, eps, alpha, one, one, one, one, None)

    def bwd(kind=0, eps=1e-3, alpha=1.0, shape=shape):
        return lib.sisr_freq_loss_bwd(one, one, one, *shape, kind, eps, alpha, one, one, one, None)
    for f in (fwd, bwd):
        assert f(eps=-1e-3) == E_BADARG and f(eps=float('nan')) == E_BADARG
        assert f(alpha=0.0) == E_BADARG and f(alpha=4.5) == E_BADARG and f(alpha=float('nan')) == E_BADARG
        assert f(kind=3) == E_BADARG and f(kind=-1) == E_BADARG
        assert f(shape=(2, 2, 45, 70, 0, 0)) == E_UNSUPPORTED
        assert f(shape=(1, 1, 257, 70, 0, 0)) == E_BADARG
        assert f(shape=(0, 3, 45, 70, 0, 0)) == E_BADARG
    assert lib.sisr_freq_loss_bwd(one, one, one, *shape, 0, 1e-3, 1.0, one, None, None, None) == E_BADARG        # no gradient asked for
    assert lib.sisr_freq_loss_fwd(one, one, *shape, 2, 1e-3, 1.0, one, one, None, one, None) == E_BADARG         # focal without pmax


@pytest.mark.parametrize('shape,crop,luma', L1_GRAD_CASES)
def test_l1_sign_margin_condition_holds_where_the_l1_gradient_is_compared(shape, crop, luma):
    assert (shape, crop, luma) in CASES
    D = _reference(shape, crop, luma, 'l1')[3]
    h, w = D.shape[-2], shape[3] - 2 * crop
    free_im = ~structural_imag_zero(h, w)
    mag = float(D.abs().max())
    assert float(D.imag.abs()[..., ~free_im].max()) <= 1e-12 * mag           # the structural zeros are zeros in the reference
    smallest = float(D.real.abs().min())
    if bool(free_im.any()):
        smallest = min(smallest, float(D.imag.abs()[..., free_im].min()))
    print('freq l1 sign margin %s crop %d luma %d: smallest component %.3g of max|D|' % (shape, crop, luma, smallest / mag))
    assert smallest >= SIGN_MARGIN * mag


@pytest.mark.parametrize('shape,crop,luma', CASES)
def test_fp32_evaluation_of_the_definition_against_float64(shape, crop, luma):
    """the floor under the GPU test's bounds, printed per case; the bounds themselves leave it a factor of about 70 (loss) and 10
    (gradient).  The L1 gradient is looked at only where the sign margin condition holds"""
    for kind in KINDS:
        l64, da64, db64, _ = _reference(shape, crop, luma, kind)
        l32, da32, db32, _ = evaluate(shape, crop, luma, kind, torch.float32)
        e_l = float(((l32.double() - l64).abs() / l64.abs()).max())
        e_g = max(float((g32.double() - g64).abs().max() / g64.abs().max()) for g32, g64 in ((da32, da64), (db32, db64)))
        print('freq fp32 definition %s crop %d luma %d %s: loss rel err %.3g, grad err %.3g of max|ref|' % (shape, crop, luma, kind, e_l, e_g))
        assert e_l <= 2e-5 / 10
        if kind != 'l1' or (shape, crop, luma) in L1_GRAD_CASES:
            assert e_g <= 1e-4 / 5
