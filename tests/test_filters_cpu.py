"""CPU: the host side of the Gaussian filter and the unsharp mask: the library's taps against the float64
formula; the float64 restatements of filters_cases.py against torch's own ops (reflect F.pad + the full K x K conv2d, its
autograd, Real-ESRGAN's USM formula); the new entry points refuse every bad argument before they touch a GPU; the Python wrappers
refuse CPU, fp64 and strided tensors."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from filters_cases import CASES, F64, NEAR, NEAR_SHARE, blur64, blur64_T, natural, noise, pkg, taps64, usm64, usm_case

BADARG, TOOBIG, UNSUPPORTED = -1, -2, -3


@pytest.mark.parametrize('sigma', [0.0, 1.5, 8.0])
@pytest.mark.parametrize('K', [1, 3, 5, 21, 51, 63])
def test_host_taps_match_the_float64_formula(K, sigma):
    t = pkg('filters').gaussian_taps(K, sigma)
    ref = taps64(K, sigma)
    err = np.abs(t.astype(np.float64) - ref).max() / ref.max()
    print('K %d sigma %g: max err / largest tap %.3e, sum - 1 %.3e' % (K, sigma, err, t.astype(np.float64).sum() - 1))
    assert t.dtype == np.float32 and t.shape == (K,)
    assert err <= 1.2e-7                                          # one fp32 rounding, doubled
    assert abs(t.astype(np.float64).sum() - 1) <= 1e-6
    assert np.array_equal(t, t[::-1])                             # symmetric bit for bit


def test_default_sigma_is_opencvs_rule():
    Fm = pkg('filters')
    assert np.array_equal(Fm.gaussian_taps(51), Fm.gaussian_taps(51, 8.0))         # 0.3 (25 - 1) + 0.8 = 8
    assert np.array_equal(Fm.gaussian_taps(51, -2.0), Fm.gaussian_taps(51, 8.0))
    assert np.array_equal(Fm.gaussian_taps(1), np.ones(1, np.float32))
    assert np.allclose(Fm.gaussian_taps(3), taps64(3, 0.8), rtol=0, atol=1e-7)      # the formula, not OpenCV's (0.25, 0.5, 0.25)


def _conv_defn(x, taps):
    """Real-ESRGAN's filter2D in float64: reflect pad + the full K x K correlation"""
    t = torch.from_numpy(np.asarray(taps, np.float64))
    K = t.numel()
    n, c, h, w = x.shape
    k2 = torch.outer(t, t).view(1, 1, K, K)
    xp = F.pad(x.reshape(n * c, 1, h, w), (K // 2,) * 4, mode='reflect')
    return F.conv2d(xp, k2).view(n, c, h, w)


@pytest.mark.parametrize('shape,K', CASES, ids=lambda v: str(v).replace(' ', ''))
def test_restatements_match_torchs_reflect_pad_and_conv(shape, K):
    taps = taps64(K)
    x = noise(shape, 1).to(F64).requires_grad_()
    g = noise(shape, 2).to(F64)
    ref = _conv_defn(x, taps)
    err = float((blur64(x.detach(), taps) - ref.detach()).abs().max())
    gx, = torch.autograd.grad(ref, x, g)
    err_t = float((blur64_T(g, taps) - gx).abs().max())
    print('%s K %d: blur64 - conv %.3e, blur64_T - autograd %.3e' % (shape, K, err, err_t))
    assert err <= 1e-12 and err_t <= 1e-12


def test_transpose_with_asymmetric_taps():
    """the restatements do not lean on the symmetry of a Gaussian"""
    taps = np.array([0.1, 0.2, 0.3, 0.15, 0.25])
    x = noise((1, 2, 6, 9), 3).to(F64).requires_grad_()
    g = noise((1, 2, 6, 9), 4).to(F64)
    ref = _conv_defn(x, taps)
    gx, = torch.autograd.grad(ref, x, g)
    assert float((blur64(x.detach(), taps) - ref.detach()).abs().max()) <= 1e-12
    assert float((blur64_T(g, taps) - gx).abs().max()) <= 1e-12


@pytest.mark.parametrize('lo,hi', [(-1.0, 1.0), (0.0, 1.0)])
def test_usm64_is_real_esrgans_formula(lo, hi):
    """USMSharp.forward of Real-ESRGAN composed from torch ops in float64 (its images live in [0, 1]: residual * 255)"""
    K, weight, threshold = 21, 0.5, 10.0
    taps = taps64(K)
    img = natural((1, 3, 40, 33), 5, 0.08).to(F64)
    img = (img + 1) / 2 * (hi - lo) + lo
    blur = _conv_defn(img, taps)
    residual = img - blur
    mask = (residual.abs() * (255 / (hi - lo)) > threshold).to(F64)
    soft_mask = _conv_defn(mask, taps)
    sharp = (img + weight * residual).clamp(lo, hi)
    want = soft_mask * sharp + (1 - soft_mask) * img
    out, own, level = usm64(img, taps, weight, threshold, lo, hi)
    assert torch.equal(own, mask) and 0.2 < float(mask.mean()) < 0.8
    assert float((out - want).abs().max()) <= 1e-12
    forced = usm64(img, taps, weight, threshold, lo, hi, mask=torch.ones_like(mask))[0]
    assert float((forced - (_conv_defn(torch.ones_like(mask), taps) * (sharp - img) + img)).abs().max()) <= 1e-12


@pytest.mark.parametrize('amp', [0.04, 0.08])
@pytest.mark.parametrize('shape,K', CASES, ids=lambda v: str(v).replace(' ', ''))
def test_usm_cases_have_few_near_ties(shape, K, amp):
    """the condition the GPU mask comparison stands on: the share of elements whose level lies within NEAR of the threshold"""
    _, _, mask, level = usm_case(shape, K, amp)
    share = float(((level - 10.0).abs() <= NEAR).to(F64).mean())
    print('%s K %d amp %g: mask fraction %.3f, near ties %.2e' % (shape, K, amp, float(mask.mean()), share))
    assert share <= NEAR_SHARE


def test_every_bad_argument_is_refused_without_a_gpu():
    lib = pkg('_lib').lib()
    buf = (C.c_float * 64)()
    # non-null pointers 16 MiB apart (the planes below are 12.8 KB): every call here is refused, refused calls never read them, and
    # nothing reaches a launch; only `p` is memory of this process (the tap entry point writes K floats there)
    p = C.cast(buf, C.c_void_p)
    q, r, m = (C.c_void_p(p.value + (i << 24)) for i in (1, 2, 3))
    n_bytes = 4 * 2 * 40 * 40

    def at(base, offset):
        return C.c_void_p(base.value + offset)
    nan, inf = float('nan'), float('inf')
    for bad in (dict(K=0), dict(K=2), dict(K=65), dict(K=-3), dict(sigma=nan), dict(sigma=inf), dict(taps=None)):
        a = dict(dict(K=5, sigma=0.0, taps=p), **bad)
        assert lib.sisr_gauss_taps_host(*a.values()) == BADARG, bad
    good = dict(x=p, taps=q, y=r, planes=2, H=40, W=40, K=51, stream=None)
    for fn in (lib.sisr_gauss_blur_fwd, lib.sisr_gauss_blur_bwd):
        for bad in (dict(x=None), dict(taps=None), dict(y=None), dict(y=p), dict(y=at(p, 4)), dict(y=at(p, n_bytes - 4)),
                    dict(y=at(p, -n_bytes + 4)), dict(y=at(q, -n_bytes + 4)), dict(y=at(q, 4 * 51 - 4)), dict(planes=0), dict(planes=-1), dict(H=0), dict(W=0),
                    dict(W=-4), dict(K=0), dict(K=2), dict(K=65), dict(K=-1)):
            assert fn(*dict(good, **bad).values()) == BADARG, bad
        for bad in (dict(H=25), dict(W=25), dict(H=1), dict(K=63, W=31)):          # H = R: the mirror needs H > R
            assert fn(*dict(good, **bad).values()) == UNSUPPORTED, bad
        assert fn(*dict(good, H=1 << 16, W=1 << 16).values()) == TOOBIG
        assert fn(*dict(good, planes=1 << 40).values()) == TOOBIG
        assert fn(*dict(good, planes=(1 << 62) + 1).values()) == TOOBIG            # planes x tiles would overflow int64
        assert fn(*dict(good, planes=(1 << 63) - 1).values()) == TOOBIG
    assert lib.sisr_usm_ws_bytes(2, 40, 40) == 5 * 2 * 40 * 40
    for bad in ((0, 4, 4), (1, 0, 4), (1, 4, -1)):
        assert lib.sisr_usm_ws_bytes(*bad) == BADARG, bad
    assert lib.sisr_usm_ws_bytes(1, 1 << 16, 1 << 16) == TOOBIG and lib.sisr_usm_ws_bytes(1 << 50, 1 << 10, 1 << 10) == TOOBIG
    good = dict(x=p, taps=q, K=51, weight=0.5, threshold=10.0, lo=-1.0, hi=1.0, ws=r, y=m, mask=None, planes=2, H=40, W=40, stream=None)
    for bad in (dict(x=None), dict(taps=None), dict(ws=None), dict(y=None), dict(y=p), dict(ws=p), dict(ws=m), dict(mask=p), dict(mask=m),
                dict(mask=r), dict(y=at(p, n_bytes - 4)), dict(y=at(q, 4)), dict(ws=at(p, -5 * n_bytes // 4 + 1)), dict(ws=at(q, 4 * 51 - 1)),
                dict(ws=at(m, n_bytes - 1)), dict(mask=at(r, n_bytes)), dict(mask=at(r, 5 * n_bytes // 4 - 1)), dict(mask=at(p, n_bytes - 1)),
                dict(mask=at(m, -n_bytes // 4 + 1)), dict(mask=at(q, 0)), dict(K=0), dict(K=2), dict(K=65), dict(lo=1.0), dict(lo=2.0), dict(hi=-1.0), dict(lo=nan), dict(hi=inf),
                dict(weight=nan), dict(threshold=inf), dict(planes=0), dict(H=0), dict(W=0)):
        assert lib.sisr_usm_fwd(*dict(good, **bad).values()) == BADARG, bad
    for bad in (dict(H=25), dict(W=25)):
        assert lib.sisr_usm_fwd(*dict(good, **bad).values()) == UNSUPPORTED, bad
    assert lib.sisr_usm_fwd(*dict(good, H=1 << 16, W=1 << 16).values()) == TOOBIG
    assert lib.sisr_usm_fwd(*dict(good, planes=(1 << 62) + 1).values()) == TOOBIG


def test_python_wrappers_validate_and_refuse_cpu_fp64_and_strided_tensors():
    Fm, top = pkg('filters'), pkg()
    assert top.gaussian_blur is Fm.gaussian_blur and top.usm_sharpen is Fm.usm_sharpen and top.USMSharp is Fm.USMSharp
    assert top.gaussian_taps is Fm.gaussian_taps
    x = torch.zeros(1, 3, 32, 32)
    for call in (lambda t: Fm.gaussian_blur(t, 21), lambda t: Fm.usm_sharpen(t, radius=20), lambda t: Fm.USMSharp(radius=20)(t)):
        with pytest.raises(RuntimeError):
            call(x)                                                # a CPU tensor: no fallback
        with pytest.raises(ValueError):
            call(x.double())
        with pytest.raises(ValueError):
            call(x.half())
        with pytest.raises(ValueError):
            call(torch.zeros(1, 3, 32, 64)[..., ::2])              # strided
        with pytest.raises(ValueError):
            call(x.transpose(2, 3))
        with pytest.raises(ValueError):
            call(x[0])                                             # not a batch
        with pytest.raises(ValueError):
            call(torch.zeros(1, 3, 10, 32))                        # H = R
        with pytest.raises(ValueError):
            call(None)
    for bad in (0, 2, 65, -1, 5.0, True):
        with pytest.raises(ValueError):
            Fm.gaussian_blur(x, bad)
        with pytest.raises(ValueError):
            Fm.gaussian_taps(bad)
    for bad in (dict(radius=0), dict(radius=64), dict(radius=2.5), dict(value_range=(1.0, 1.0)), dict(value_range=(1.0, -1.0)),
                dict(weight=float('nan')), dict(threshold=float('inf')), dict(sigma=float('nan'))):
        with pytest.raises(ValueError):
            Fm.usm_sharpen(x, **bad)
    usm = Fm.USMSharp()
    assert (usm.radius, usm.sigma, usm.value_range) == (50, 0, (-1, 1)) and not list(usm.parameters())
