"""Randomised blur + noise degradation on the device (csrc/degrade.hip).

The reference's only HR -> LR operator is ``utils.lr_from_hr``: bicubic resampling and a clamp.  The classical super-resolution
measurement model is wider -- ``LR = clamp((HR (*) k) resampled + sigma_n z)`` with a blur kernel and a noise level of the sample's
own -- and a generator trained against bicubic alone is known to fail on images that were not bicubically downsampled.

>>> d = Degrader(ksize=21, sigma=(0.2, 3.0), anisotropic=True, noise=(0., 0.05), seed=1)
>>> img_lr = d(img_hr, (48, 48))                       # draw + forward: two launches, differentiable in img_hr, capturable
>>> sisr.install(degradation=d)                        # the reference's utils.lr_from_hr now draws
>>> d = Degrader(noise=(0., 0.05), jpeg=(30, 95))      # ... and ends with a JPEG round trip at a random quality (jpeg.py)

``degrade`` is the operator with the kernels given; ``gaussian_kernels`` builds fixed ones; ``expected_params`` / ``expected_noise``
restate a step's draws on the host (no GPU) for audits and tests.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib as L
from .engine import _stream, require_gpu_tensor

KSIZE_MAX = 21
RANK_LIMIT = 1 << 16


def _check_ksize(ksize, who):
    ksize = int(ksize)
    if not 1 <= ksize <= KSIZE_MAX or ksize % 2 == 0:
        raise ValueError('%s: ksize must be odd and in [1, %d], got %d' % (who, KSIZE_MAX, ksize))
    return ksize


class _Degrade(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, size, kernels, noise_sigma, step, seed, rank, clamp):
        n, c, h, w = x.shape
        oh, ow = size
        K = kernels.shape[-1]
        y = torch.empty((n, c, oh, ow), dtype=torch.float32, device=x.device)
        L.check(L.lib().sisr_degrade_fwd(x.data_ptr(), kernels.data_ptr(), None if noise_sigma is None else noise_sigma.data_ptr(),
                                         None if step is None else step.data_ptr(), seed, rank, y.data_ptr(), n, c, h, w, K, oh, ow,
                                         int(clamp), _stream()), 'sisr_degrade_fwd')
        ctx.shape, ctx.clamp = (n, c, h, w, K, oh, ow), clamp
        ctx.save_for_backward(kernels, *((y,) if clamp else ()))
        return y

    @staticmethod
    def backward(ctx, dy):
        n, c, h, w, K, oh, ow = ctx.shape
        dy = dy.contiguous()
        kernels = ctx.saved_tensors[0]
        yc = ctx.saved_tensors[1] if ctx.clamp else None
        dx = torch.empty((n, c, h, w), dtype=torch.float32, device=dy.device)
        L.check(L.lib().sisr_degrade_bwd(dy.data_ptr(), None if yc is None else yc.data_ptr(), kernels.data_ptr(), dx.data_ptr(),
                                         n, c, h, w, K, oh, ow, _stream()), 'sisr_degrade_bwd')
        return (dx,) + (None,) * 7


def degrade(img_hr, image_size_lr, kernels, noise_sigma=None, step=None, seed=0, rank=0, clamp=True):
    """``clamp(bicubic(img_hr (*) kernels) + noise_sigma z)``: img_hr [N, C, H, W] fp32 on the device, C in 1..4 -> [N, C, h, w].

    ``kernels``      [N, K, K] (or [K, K] for every sample), K odd <= 21; correlated with the image over a replicate border, used
                     as given -- NOT renormalised.
    ``noise_sigma``  [N] standard deviations, or None for no noise.  z is standard normal, a pure function of (seed, rank, the step
                     count, the output element): ``expected_noise`` restates it.  A constant under autograd.
    ``step``         the step count the noise is drawn for: a 0-dim int64 DEVICE tensor (read by the kernel: a captured call
                     follows it) or a host int; None: 0.
    Differentiable in ``img_hr`` alone; the backward pass is deterministic (gather form, no atomics)."""
    require_gpu_tensor(img_hr, 'degrade input')
    if img_hr.dim() != 4 or not 1 <= img_hr.shape[1] <= 4:
        raise ValueError('degrade: an [N, C, H, W] batch with 1 to 4 channels is expected, got %s' % (tuple(img_hr.shape),))
    x = img_hr.contiguous()
    n = x.shape[0]
    size = (int(image_size_lr[0]), int(image_size_lr[1]))
    if min(size) < 1:
        raise ValueError('degrade: the output size must be >= 1, got %s' % (size,))
    k = torch.as_tensor(kernels).to(device=x.device, dtype=torch.float32)
    if k.dim() == 2:
        k = k.expand(n, -1, -1)
    if k.dim() != 3 or k.shape[0] != n or k.shape[1] != k.shape[2]:
        raise ValueError('degrade: kernels must be [N = %d, K, K] or [K, K], got %s' % (n, tuple(k.shape)))
    _check_ksize(k.shape[-1], 'degrade')
    seed, rank = int(seed), int(rank)
    if not 0 <= seed < 1 << 64 or not 0 <= rank < RANK_LIMIT:
        raise ValueError('degrade: seed must be in [0, 2^64) and rank in [0, %d), got %d, %d' % (RANK_LIMIT, seed, rank))
    if noise_sigma is not None:
        noise_sigma = torch.as_tensor(noise_sigma).to(device=x.device, dtype=torch.float32).contiguous()
        if noise_sigma.dim() != 1 or noise_sigma.shape[0] != n:
            raise ValueError('degrade: noise_sigma must be [N = %d], got %s' % (n, tuple(noise_sigma.shape)))
        if not (isinstance(step, torch.Tensor) and step.is_cuda and step.dtype == torch.int64 and step.numel() == 1):
            step = torch.full((), 0 if step is None else int(step), dtype=torch.int64, device=x.device)
    else:
        step = None
    return _Degrade.apply(x, size, k.contiguous(), noise_sigma, step, seed, rank, bool(clamp))


def gaussian_kernels(sigma1, sigma2, theta, ksize):
    """Fixed kernels from explicit parameters, computed in float64: weight(dy, dx) = exp(-(u^2 / sigma1^2 + v^2 / sigma2^2) / 2) with
    u = cos(theta) dx + sin(theta) dy, v = -sin(theta) dx + cos(theta) dy, divided by the kernel's sum.  The three parameters are
    scalars or [N] sequences (broadcast) -> float64 tensor [N, ksize, ksize] on the host."""
    ksize = _check_ksize(ksize, 'gaussian_kernels')
    s1, s2, th = np.broadcast_arrays(*(np.atleast_1d(np.asarray(torch.as_tensor(v).cpu() if isinstance(v, torch.Tensor) else v,
                                                                 dtype=np.float64)) for v in (sigma1, sigma2, theta)))
    if s1.ndim != 1 or (s1 <= 0).any() or (s2 <= 0).any():
        raise ValueError('gaussian_kernels: scalars or [N] sequences with sigma > 0 are expected')
    r = np.arange(ksize, dtype=np.float64) - (ksize - 1) // 2
    dy, dx = r[None, :, None], r[None, None, :]
    cs, sn = np.cos(th)[:, None, None], np.sin(th)[:, None, None]
    u, v = cs * dx + sn * dy, -sn * dx + cs * dy
    wgt = np.exp(-0.5 * (u * u / (s1 * s1)[:, None, None] + v * v / (s2 * s2)[:, None, None]))
    return torch.from_numpy(wgt / wgt.sum(axis=(1, 2), keepdims=True))


def _check_ranges(sigma, noise, who):
    lo, hi, nlo, nhi = float(sigma[0]), float(sigma[1]), float(noise[0]), float(noise[1])
    if not (0.0 < lo <= hi < math.inf):
        raise ValueError('%s: sigma = (lo, hi) needs 0 < lo <= hi, got (%g, %g)' % (who, lo, hi))
    if not (0.0 <= nlo <= nhi < math.inf):
        raise ValueError('%s: noise = (lo, hi) needs 0 <= lo <= hi, got (%g, %g)' % (who, nlo, nhi))
    return lo, hi, nlo, nhi


def expected_params(seed, t, B, ksize, sigma=(0.2, 3.0), anisotropic=True, noise=(0., 0.), rank=0):
    """Host, no GPU (sisr_degrade_params_host: the device code's own text compiled for the host): the draw of step ``t`` ->
    (kernels [B, K, K], noise_sigma [B], params [B, 4] = sigma1, sigma2, theta, sigma_n), float32 numpy arrays."""
    B, ksize = int(B), _check_ksize(ksize, 'expected_params')
    lo, hi, nlo, nhi = _check_ranges(sigma, noise, 'expected_params')
    if B < 1 or int(t) < 0:
        raise ValueError('expected_params: B must be >= 1 and t >= 0, got %d, %d' % (B, int(t)))
    k, s, p = np.zeros((B, ksize, ksize), np.float32), np.zeros(B, np.float32), np.zeros((B, 4), np.float32)
    L.check(L.lib().sisr_degrade_params_host(int(t), int(seed), int(rank), B, ksize, lo, hi, int(bool(anisotropic)), nlo, nhi,
                                             k.ctypes.data_as(C.c_void_p), s.ctypes.data_as(C.c_void_p), p.ctypes.data_as(C.c_void_p)),
            'sisr_degrade_params_host')
    return k, s, p


def expected_noise(seed, t, first, count, rank=0):
    """Host, no GPU (sisr_degrade_noise_host): z of output elements ``first`` .. ``first + count - 1`` (flat over [N, C, h, w]) at
    step ``t`` -> float32 numpy array [count]."""
    z = np.zeros(int(count), np.float32)
    L.check(L.lib().sisr_degrade_noise_host(int(t), int(seed), int(rank), int(first), int(count), z.ctypes.data_as(C.c_void_p)),
            'sisr_degrade_noise_host')
    return z


class Degrader:
    """A new blur kernel and noise level per sample and per call, drawn on the device.

    ``sigma``        (lo, hi): the two standard deviations of the Gaussian kernel are uniform in it (``anisotropic=False``: one
                     for both axes); its orientation is uniform in [0, pi).  The kernel is normalised to sum 1.
    ``noise``        (lo, hi): the noise standard deviation is uniform in it; (0, 0) switches the noise off altogether.
    ``seed, rank``   key and stream of the Philox4x32-10 draws (rank < 65536: one stream per data-parallel rank).
    ``jpeg``         None, or (qlo, qhi): the LR image additionally goes through ``jpeg.jpeg_roundtrip`` at a quality uniform in
                     qlo .. qhi per sample, with ``jpeg_subsampling`` ('420' / '444') and the rounding surrogate ``jpeg_grad``
                     ('ste' / 'cubic').  The call is then four launches -- sisr_degrade_draw, sisr_jpeg_tables (on the SAME step:
                     the count advances once, ``state_dict`` is unchanged), sisr_degrade_fwd, sisr_jpeg_fwd -- still nothing read
                     back; ``last_quality`` [N] int32 and ``last_tables`` [N, 2, 8, 8] are the latest call's.

    ``d(img_hr, image_size_lr)`` is two launches -- sisr_degrade_draw, sisr_degrade_fwd -- and reads nothing back: the step count is
    device memory that the draw advances, so a call captured by graph.GraphedStep degrades differently on every replay.  Every
    call draws its own tables (two calls before one backward pass, as the reference's unsupervised branch makes for ``img_hr`` and
    ``fake``, keep their own kernels); ``last_kernels`` [N, K, K] and ``last_noise_sigma`` [N] are the latest call's.  ``step`` is
    the 0-dim int64 device tensor of draws made so far."""

    def __init__(self, ksize=21, sigma=(0.2, 3.0), anisotropic=True, noise=(0., 0.), seed=0, rank=0, device=None, jpeg=None,
                 jpeg_subsampling='420', jpeg_grad='ste'):
        self.ksize = _check_ksize(ksize, 'Degrader')
        self.sigma_lo, self.sigma_hi, self.noise_lo, self.noise_hi = _check_ranges(sigma, noise, 'Degrader')
        self.anisotropic, self.seed, self.rank = bool(anisotropic), int(seed), int(rank)
        if not 0 <= self.seed < 1 << 64 or not 0 <= self.rank < RANK_LIMIT:
            raise ValueError('Degrader: seed must be in [0, 2^64) and rank in [0, %d), got %d, %d' % (RANK_LIMIT, self.seed, self.rank))
        self.jpeg = None
        if jpeg is not None:
            from . import jpeg as J
            qlo, qhi = int(jpeg[0]), int(jpeg[1])
            if not 1 <= qlo <= qhi <= 100:
                raise ValueError('Degrader: jpeg = (qlo, qhi) needs 1 <= qlo <= qhi <= 100, got (%d, %d)' % (qlo, qhi))
            if jpeg_subsampling not in J.SUBSAMPLING or jpeg_grad not in J.GRAD:
                raise ValueError("Degrader: jpeg_subsampling is '444' or '420' and jpeg_grad 'ste' or 'cubic', got %r, %r"
                                 % (jpeg_subsampling, jpeg_grad))
            self.jpeg, self.jpeg_subsampling, self.jpeg_grad = (qlo, qhi), jpeg_subsampling, jpeg_grad
        dev = torch.device('cuda' if device is None else device)
        if dev.type != 'cuda':
            raise RuntimeError('Degrader: the draws live on the MI355X (got device %s); there is no CPU fallback' % dev)
        self.step = torch.zeros((), dtype=torch.int64, device=dev)
        self.last_kernels = self.last_noise_sigma = self.last_drawn_step = self.last_quality = self.last_tables = None

    def draw(self, n):
        """the tables of the next step for a batch of ``n``: -> (kernels, noise_sigma, drawn_step) on the device; advances ``step``"""
        dev = self.step.device
        k = torch.empty((n, self.ksize, self.ksize), dtype=torch.float32, device=dev)
        s = torch.empty(n, dtype=torch.float32, device=dev)
        t = torch.empty((), dtype=torch.int64, device=dev)
        L.check(L.lib().sisr_degrade_draw(self.step.data_ptr(), self.seed, self.rank, n, self.ksize, self.sigma_lo, self.sigma_hi,
                                          int(self.anisotropic), self.noise_lo, self.noise_hi, k.data_ptr(), s.data_ptr(),
                                          t.data_ptr(), _stream()), 'sisr_degrade_draw')
        self.last_kernels, self.last_noise_sigma, self.last_drawn_step = k, s, t
        return k, s, t

    def __call__(self, img_hr, image_size_lr):
        require_gpu_tensor(img_hr, 'Degrader input')
        if img_hr.device != self.step.device:
            raise RuntimeError('Degrader: the batch is on %s, the draws on %s' % (img_hr.device, self.step.device))
        k, s, t = self.draw(int(img_hr.shape[0]))
        noisy = self.noise_hi > 0.0
        if self.jpeg is None:
            return degrade(img_hr, image_size_lr, k, s if noisy else None, t if noisy else None, self.seed, self.rank, True)
        tables = self.draw_jpeg_tables(int(img_hr.shape[0]), t)          # before the forward: the draws of a step stay together
        lr = degrade(img_hr, image_size_lr, k, s if noisy else None, t if noisy else None, self.seed, self.rank, True)
        from .jpeg import jpeg_roundtrip
        return jpeg_roundtrip(lr, tables, self.jpeg_subsampling, self.jpeg_grad, True)

    def draw_jpeg_tables(self, n, drawn_step):
        """the quantisation tables of step ``drawn_step`` (a 0-dim int64 device tensor, read and NOT advanced) for a batch of ``n``
        -> tables [n, 2, 8, 8] on the device; ``last_quality`` holds the qualities"""
        dev = self.step.device
        q = torch.empty(n, dtype=torch.int32, device=dev)
        tables = torch.empty((n, 2, 8, 8), dtype=torch.float32, device=dev)
        L.check(L.lib().sisr_jpeg_tables(drawn_step.data_ptr(), self.seed, self.rank, n, self.jpeg[0], self.jpeg[1], q.data_ptr(),
                                         tables.data_ptr(), _stream()), 'sisr_jpeg_tables')
        self.last_quality, self.last_tables = q, tables
        return tables

    def lr_from_hr(self, img_hr, image_size_lr, device='cpu'):
        """the reference's signature (utils.py:22-31; ``device`` is accepted and unused, as in utils.lr_from_hr)"""
        return self(img_hr, image_size_lr)

    def state_dict(self):
        return dict(seed=self.seed, rank=self.rank, step=self.step.clone())

    def load_state_dict(self, state):
        """copies the count INTO the existing tensor (a captured draw points at it)"""
        seed, rank = int(state['seed']), int(state['rank'])
        if not 0 <= seed < 1 << 64 or not 0 <= rank < RANK_LIMIT:
            raise ValueError('Degrader.load_state_dict: seed must be in [0, 2^64) and rank in [0, %d), got %d, %d' % (RANK_LIMIT, seed, rank))
        self.step.copy_(torch.as_tensor(state['step'], dtype=torch.int64).reshape(()))
        self.seed, self.rank = seed, rank
