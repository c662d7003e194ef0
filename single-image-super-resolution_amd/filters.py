"""A separable Gaussian filter with a mirrored border and Real-ESRGAN's unsharp mask (USM) on the device (csrc/gauss.hip;
DESIGN.md section 26).

``gaussian_blur(x, ksize, sigma)`` filters every plane of an fp32 [N, C, H, W] batch with the ``ksize``-tap Gaussian along both
axes; the border is mirrored without repeating the edge pixel (torch's ``reflect``, OpenCV's ``BORDER_REFLECT_101``, what
Real-ESRGAN's ``filter2D`` pads with), so both sides must be longer than ``ksize // 2``.  One launch forward and one backward
(the exact transpose, gathered: no atomics, the same bits on every call); nothing is saved, the operator is linear.  The taps are
``exp(-(i - (K - 1) / 2)^2 / (2 sigma^2))`` normalised in double; ``sigma <= 0`` takes OpenCV's rule
``0.3 ((K - 1) / 2 - 1) + 0.8`` with that formula for EVERY size: OpenCV's tabulated kernels for ``ksize <= 7`` are not reproduced.

With it the low-pass L1 and a blurred colour-consistency term are compositions::

    loss = l1_loss(gaussian_blur(sr, 21), gaussian_blur(hr, 21))

``usm_sharpen`` / ``USMSharp`` build the sharpened training target of Real-ESRGAN: two launches, no gradient (the target carries
none).  The reference's ``train.py`` has no hook for the target, so ``install()`` does not touch it; a trainer that degrades with
``degrade.HighOrderDegrader`` adds two lines, degrading the UNSHARPENED patch and training against the sharpened one::

    usm = USMSharp()
    ...
    lr = d.lr_from_hr(hr, size); hr = usm(hr)

Nothing here synchronises with the host.  The device copy of a tap vector is made on first use per (ksize, sigma, device) -- a
host-to-device copy, so call once before capturing a graph (a warm-up does).  No CPU path: CPU tensors are refused.
"""
import ctypes as C

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _lib as L
from .engine import _stream, require_gpu_tensor
from .losses import _check_tensor

_TAPS = {}           # (ksize, sigma, device) -> the taps in device memory


def _check_ksize(ksize, what):
    if not isinstance(ksize, int) or isinstance(ksize, bool) or ksize < 1 or ksize > L.GAUSS_MAX_K or ksize % 2 == 0:
        raise ValueError('%s: the size is an odd integer in 1 .. %d, got %r' % (what, L.GAUSS_MAX_K, ksize))
    return ksize


def _check_sigma(sigma, what):
    sigma = float(sigma)
    if not np.isfinite(sigma):
        raise ValueError('%s: sigma must be finite, got %r' % (what, sigma))
    return sigma


def gaussian_taps(ksize, sigma=0.0):
    """the ``ksize`` taps as a numpy fp32 array, from the library's host entry point; ``sigma <= 0``: OpenCV's rule (8.0 at 51)
    with the formula for every size (OpenCV's tabulated kernels for ``ksize <= 7`` are not reproduced)"""
    ksize, sigma = _check_ksize(ksize, 'gaussian_taps'), _check_sigma(sigma, 'gaussian_taps')
    taps = np.zeros(ksize, np.float32)
    L.check(L.lib().sisr_gauss_taps_host(ksize, sigma, taps.ctypes.data_as(C.c_void_p)), 'sisr_gauss_taps_host')
    return taps


def _device_taps(ksize, sigma, device):
    key = (ksize, sigma, device)
    t = _TAPS.get(key)
    if t is None:
        t = _TAPS[key] = torch.from_numpy(gaussian_taps(ksize, sigma)).to(device)
    return t


def _check_image(x, ksize, what):
    """argument errors first, whatever the tensor lives on; then the device"""
    _check_tensor(x, what)
    if x.dim() != 4:
        raise ValueError('%s: an [N, C, H, W] batch is expected, got shape %s' % (what, tuple(x.shape)))
    if not x.is_contiguous():
        raise ValueError('%s: a contiguous tensor is expected, got strides %s for shape %s' % (what, x.stride(), tuple(x.shape)))
    h, w = x.shape[-2:]
    if min(h, w) <= ksize // 2:
        raise ValueError('%s: the mirrored border of a %d-tap filter needs sides longer than %d, got %d x %d'
                         % (what, ksize, ksize // 2, h, w))
    require_gpu_tensor(x, what)


class _GaussianBlur(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, ksize, sigma):
        x = x.detach()
        n, c, h, w = x.shape
        taps, y = _device_taps(ksize, sigma, x.device), torch.empty_like(x)
        L.check(L.lib().sisr_gauss_blur_fwd(x.data_ptr(), taps.data_ptr(), y.data_ptr(), n * c, h, w, ksize, _stream()),
                'sisr_gauss_blur_fwd')
        ctx.cfg = (ksize, sigma)               # nothing is saved: the operator is linear
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        ksize, sigma = ctx.cfg
        g = g.to(torch.float32).contiguous()
        n, c, h, w = g.shape
        taps, dx = _device_taps(ksize, sigma, g.device), torch.empty_like(g)
        L.check(L.lib().sisr_gauss_blur_bwd(g.data_ptr(), taps.data_ptr(), dx.data_ptr(), n * c, h, w, ksize, _stream()),
                'sisr_gauss_blur_bwd')
        return dx, None, None


def gaussian_blur(x, ksize, sigma=0.0):
    """The ``ksize``-tap Gaussian along both axes of every plane of an fp32 [N, C, H, W] device batch, mirrored border (see the
    module text) -> a tensor of the same shape.  Differentiable with respect to ``x``, once.  ``ksize`` odd, 1 .. 63; H and W
    longer than ``ksize // 2``.  CPU, non-fp32 and non-contiguous tensors are refused."""
    ksize, sigma = _check_ksize(ksize, 'gaussian_blur'), _check_sigma(sigma, 'gaussian_blur')
    _check_image(x, ksize, 'gaussian_blur')
    return _GaussianBlur.apply(x, ksize, sigma)


def usm_sharpen(img, weight=0.5, radius=50, threshold=10.0, sigma=0.0, value_range=(-1.0, 1.0), return_mask=False):
    """Real-ESRGAN's ``USMSharp`` on an fp32 [N, C, H, W] device batch with values in ``value_range`` = (lo, hi)::

        blur  = G * img                                   G: the ``radius``-tap Gaussian of ``gaussian_blur`` (an even radius
        res   = img - blur                                   becomes radius + 1, as in Real-ESRGAN: 50 -> 51 taps, sigma 8)
        mask  = |res| * 255 / (hi - lo) > threshold       (0 / 1)
        soft  = G * mask
        sharp = clip(img + weight * res, lo, hi)
        out   = img + soft * (sharp - img)                = soft * sharp + (1 - soft) * img

    The last line is written so that ``weight = 0`` or an all-zero mask returns ``img`` bit for bit.  Two launches.  It runs
    without autograd and the result never requires a gradient: the target of a loss carries none.  ``return_mask=True`` ->
    ``(out, mask)`` with the uint8 mask.  CPU, non-fp32 and non-contiguous tensors are refused."""
    what = 'usm_sharpen'
    if not isinstance(radius, int) or isinstance(radius, bool) or radius < 1:
        raise ValueError('%s: the radius is a positive integer, got %r' % (what, radius))
    ksize = _check_ksize(radius + 1 if radius % 2 == 0 else radius, what)
    sigma, weight, threshold = _check_sigma(sigma, what), float(weight), float(threshold)
    lo, hi = (float(v) for v in value_range)
    if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi):
        raise ValueError('%s: value_range is (lo, hi) with lo < hi, got %r' % (what, (lo, hi)))
    if not (np.isfinite(weight) and np.isfinite(threshold)):
        raise ValueError('%s: weight and threshold must be finite, got %r and %r' % (what, weight, threshold))
    _check_image(img, ksize, what)
    with torch.no_grad():
        x = img.detach()
        n, c, h, w = x.shape
        lib = L.lib()
        ws = torch.empty(L.check_count(lib.sisr_usm_ws_bytes(n * c, h, w), 'sisr_usm_ws_bytes'), dtype=torch.uint8, device=x.device)
        taps, y = _device_taps(ksize, sigma, x.device), torch.empty_like(x)
        mask = torch.empty(x.shape, dtype=torch.uint8, device=x.device) if return_mask else None
        L.check(lib.sisr_usm_fwd(x.data_ptr(), taps.data_ptr(), ksize, weight, threshold, lo, hi, ws.data_ptr(), y.data_ptr(),
                                 None if mask is None else mask.data_ptr(), n * c, h, w, _stream()), 'sisr_usm_fwd')
    return (y, mask) if return_mask else y


class USMSharp(torch.nn.Module):
    """Real-ESRGAN's ``USMSharp(radius=50, sigma=0)`` with its ``forward(img, weight=0.5, threshold=10)``, on ``usm_sharpen``;
    ``value_range``: the range the images live in ((-1, 1) for this trainer, (0, 1) for Real-ESRGAN's own tensors)"""

    def __init__(self, radius=50, sigma=0, value_range=(-1, 1)):
        super().__init__()
        self.radius, self.sigma, self.value_range = radius, sigma, tuple(value_range)

    def forward(self, img, weight=0.5, threshold=10):
        return usm_sharpen(img, weight, self.radius, threshold, self.sigma, self.value_range)
