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

>>> d = HighOrderDegrader(mid_size=(136, 136), seed=1)  # Real-ESRGAN's two stages: seven kernel families, shot noise, JPEG, sinc

The second-order model is at the end of the file: ``DegradeStage`` / ``realesrgan_stages``,
``degrade_noise``, ``expected_mix`` and ``HighOrderDegrader``.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib as L
from . import jpeg as J
from .draws import DrawStream, check_seed_rank, step_tensor
from .engine import _stream, require_gpu_tensor

KSIZE_MAX = 21


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
    seed, rank = check_seed_rank(seed, rank, 'degrade')
    if noise_sigma is not None:
        noise_sigma = torch.as_tensor(noise_sigma).to(device=x.device, dtype=torch.float32).contiguous()
        if noise_sigma.dim() != 1 or noise_sigma.shape[0] != n:
            raise ValueError('degrade: noise_sigma must be [N = %d], got %s' % (n, tuple(noise_sigma.shape)))
        step = step_tensor(step, x.device)
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


def _check_range(r, who, name, positive):
    lo, hi = float(r[0]), float(r[1])
    if not ((0.0 < lo if positive else 0.0 <= lo) and lo <= hi < math.inf):
        raise ValueError('%s: %s = (lo, hi) needs %s lo <= hi, got (%g, %g)' % (who, name, '0 <' if positive else '0 <=', lo, hi))
    return lo, hi


def _check_ranges(sigma, noise, who):
    return _check_range(sigma, who, 'sigma', True) + _check_range(noise, who, 'noise', False)


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


def expected_noise(seed, t, first, count, rank=0, grey=False):
    """Host, no GPU (sisr_degrade_noise_host): z of output elements ``first`` .. ``first + count - 1`` (flat over [N, C, h, w]) at
    step ``t`` -> float32 numpy array [count].  ``grey=True``: the stream of ``degrade_noise``'s grey mode, one z per PIXEL (flat
    over [N, h, w]; sisr_degrade_noise_grey_host)."""
    z = np.zeros(int(count), np.float32)
    fn = 'sisr_degrade_noise_grey_host' if grey else 'sisr_degrade_noise_host'
    L.check(getattr(L.lib(), fn)(int(t), int(seed), int(rank), int(first), int(count), z.ctypes.data_as(C.c_void_p)), fn)
    return z


class Degrader(DrawStream):
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
        self.anisotropic = bool(anisotropic)
        self.jpeg = None
        if jpeg is not None:
            self.jpeg = J.check_quality_range(jpeg, 'Degrader')
            if jpeg_subsampling not in J.SUBSAMPLING or jpeg_grad not in J.GRAD:
                raise ValueError("Degrader: jpeg_subsampling is '444' or '420' and jpeg_grad 'ste' or 'cubic', got %r, %r"
                                 % (jpeg_subsampling, jpeg_grad))
            self.jpeg_subsampling, self.jpeg_grad = jpeg_subsampling, jpeg_grad
        self._init_stream(seed, rank, device)
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
        # before the forward: the draws of a step stay together
        tables = None if self.jpeg is None else self.draw_jpeg_tables(int(img_hr.shape[0]), t)
        lr = degrade(img_hr, image_size_lr, k, s if noisy else None, t if noisy else None, self.seed, self.rank, True)
        return lr if tables is None else J.jpeg_roundtrip(lr, tables, self.jpeg_subsampling, self.jpeg_grad, True)

    def draw_jpeg_tables(self, n, drawn_step):
        """the quantisation tables of step ``drawn_step`` (a 0-dim int64 device tensor, read and NOT advanced) for a batch of ``n``
        -> tables [n, 2, 8, 8] on the device; ``last_quality`` holds the qualities"""
        self.last_quality, self.last_tables = J.draw_tables(drawn_step, self.seed, self.rank, n, *self.jpeg)
        return self.last_tables

    def lr_from_hr(self, img_hr, image_size_lr, device='cpu'):
        """the reference's signature (utils.py:22-31; ``device`` is accepted and unused, as in utils.lr_from_hr)"""
        return self(img_hr, image_size_lr)


# ---- second-order degradation ------------------------------------------------------------------------------
FAMILIES = ('iso', 'aniso', 'generalized_iso', 'generalized_aniso', 'plateau_iso', 'plateau_aniso', 'sinc')
NOISE_MODES = ('none', 'gaussian', 'shot')


def _check_prob(p, who, name):
    p = float(p)
    if not 0.0 <= p <= 1.0:
        raise ValueError('%s: %s must be a probability in [0, 1], got %g' % (who, name, p))
    return p


class DegradeStage:
    """The settings of one stage of ``HighOrderDegrader``: the blur kernel is drawn from seven families, the noise is Gaussian or
    shot noise, colour or grey, and the stage may end with a JPEG round trip.

    ``ksize, ksize_min``   the kernel table is ksize x ksize (odd, <= 21); the drawn kernel occupies a centred square whose odd side
                           is uniform in ksize_min .. ksize, the rest of the table is 0.
    ``blur_prob``          the probability of blurring at all (otherwise the delta kernel).
    ``sinc_prob``          the probability of the sinc family; otherwise ``kernel_probs`` picks among iso, aniso, generalized_iso,
                           generalized_aniso, plateau_iso, plateau_aniso (six values >= 0 that sum to 1).
    ``sigma``              both standard deviations are uniform in it; ``beta_gaussian`` / ``beta_plateau`` likewise for the shape.
    ``noise, shot``        amplitude ranges of the two noise modes in [-1, 1] units (``shot``: Real-ESRGAN's poisson_scale);
                           Gaussian with probability ``gaussian_prob``, grey with ``grey_prob``; both (0, 0): no noise.
    ``jpeg``               None or (qlo, qhi)."""

    def __init__(self, ksize=21, ksize_min=7, blur_prob=1.0, kernel_probs=(0.45, 0.25, 0.12, 0.03, 0.12, 0.03), sinc_prob=0.1,
                 sigma=(0.2, 3.0), beta_gaussian=(0.5, 4.0), beta_plateau=(1.0, 2.0), noise=(0., 0.), shot=(0., 0.), gaussian_prob=0.5,
                 grey_prob=0.4, jpeg=None):
        who = 'DegradeStage'
        self.ksize, self.ksize_min = _check_ksize(ksize, who), int(ksize_min)
        if not 1 <= self.ksize_min <= self.ksize or self.ksize_min % 2 == 0:
            raise ValueError('%s: ksize_min must be odd and in [1, ksize = %d], got %d' % (who, self.ksize, self.ksize_min))
        self.blur_prob, self.sinc_prob = _check_prob(blur_prob, who, 'blur_prob'), _check_prob(sinc_prob, who, 'sinc_prob')
        self.gaussian_prob, self.grey_prob = _check_prob(gaussian_prob, who, 'gaussian_prob'), _check_prob(grey_prob, who, 'grey_prob')
        self.kernel_probs = tuple(float(p) for p in kernel_probs)
        if len(self.kernel_probs) != 6 or min(self.kernel_probs) < 0 or abs(sum(self.kernel_probs) - 1.0) > 1e-6:
            raise ValueError('%s: kernel_probs must be six values >= 0 that sum to 1, got %s' % (who, self.kernel_probs))
        self.sigma = _check_range(sigma, who, 'sigma', True)
        self.beta_gaussian = _check_range(beta_gaussian, who, 'beta_gaussian', True)
        self.beta_plateau = _check_range(beta_plateau, who, 'beta_plateau', True)
        self.noise, self.shot = _check_range(noise, who, 'noise', False), _check_range(shot, who, 'shot', False)
        self.jpeg = None if jpeg is None else J.check_quality_range(jpeg, who)

    def c_struct(self, final_sinc_prob=None):
        """the settings as sisr_hip.h's SisrDegradeMix"""
        fp = 0.0 if final_sinc_prob is None else _check_prob(final_sinc_prob, 'DegradeStage', 'final_sinc_prob')
        return L.DegradeMix(self.ksize, self.ksize_min, self.blur_prob, self.sinc_prob, (C.c_float * 6)(*self.kernel_probs), *self.sigma,
                            *self.beta_gaussian, *self.beta_plateau, *self.noise, *self.shot, self.gaussian_prob, self.grey_prob, fp)


def realesrgan_stages():
    """The two published stages of Real-ESRGAN's second-order model in this package's units: noise 1-30 / 1-25 of 255 (times 2 for
    the [-1, 1] range), poisson_scale 0.05-3 / 0.05-2.5, JPEG quality 30-95, blur probability 1.0 / 0.8, sigma (0.2, 3) / (0.2, 1.5)."""
    return (DegradeStage(blur_prob=1.0, sigma=(0.2, 3.0), noise=(2 / 255., 60 / 255.), shot=(0.05, 3.0), jpeg=(30, 95)),
            DegradeStage(blur_prob=0.8, sigma=(0.2, 1.5), noise=(2 / 255., 50 / 255.), shot=(0.05, 2.5), jpeg=(30, 95)))


def expected_mix(seed, t, B, stage, rank=0, final_sinc_prob=None):
    """Host, no GPU (sisr_degrade_mix_host: the device code's own text compiled for the host): the mixed draw of step ``t`` ->
    (kernels [B, K, K], final_kernels [B, K, K] or None, params [B, 8] = family, k_eff, sigma1, sigma2, theta, beta, omega, blur
    flag, noise_table [B, 4] = mode, grey flag, amplitude, 0), float32 numpy arrays.  ``final_sinc_prob=None``: no final filter."""
    B, K = int(B), stage.ksize
    if B < 1 or int(t) < 0:
        raise ValueError('expected_mix: B must be >= 1 and t >= 0, got %d, %d' % (B, int(t)))
    mix = stage.c_struct(final_sinc_prob)
    k, p, nt = np.zeros((B, K, K), np.float32), np.zeros((B, 8), np.float32), np.zeros((B, 4), np.float32)
    fk = None if final_sinc_prob is None else np.zeros((B, K, K), np.float32)
    L.check(L.lib().sisr_degrade_mix_host(int(t), int(seed), int(rank), B, C.byref(mix), k.ctypes.data_as(C.c_void_p),
                                          None if fk is None else fk.ctypes.data_as(C.c_void_p), p.ctypes.data_as(C.c_void_p),
                                          nt.ctypes.data_as(C.c_void_p)), 'sisr_degrade_mix_host')
    return k, fk, p, nt


class _DegradeNoise(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, table, step, seed, rank, clamp):
        n, c, h, w = x.shape
        y = torch.empty_like(x)
        L.check(L.lib().sisr_degrade_noise_fwd(x.data_ptr(), table.data_ptr(), step.data_ptr(), seed, rank, y.data_ptr(), n, c, h, w,
                                               int(clamp), _stream()), 'sisr_degrade_noise_fwd')
        ctx.shape, ctx.clamp = (n, c, h, w), clamp
        ctx.save_for_backward(*((y,) if clamp else ()))
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        yc = ctx.saved_tensors[0] if ctx.clamp else None
        dx = torch.empty_like(dy)
        L.check(L.lib().sisr_degrade_noise_bwd(dy.data_ptr(), None if yc is None else yc.data_ptr(), dx.data_ptr(), *ctx.shape,
                                               _stream()), 'sisr_degrade_noise_bwd')
        return (dx,) + (None,) * 5


def degrade_noise(x, noise_table, step, seed=0, rank=0, clamp=True):
    """``clamp(x + n)`` over x [N, C, h, w] fp32 on the device, C in 1..4, with the noise of each sample's row of ``noise_table``
    [N, 4] = (mode, grey flag, amplitude a, 0):

    mode 0 ``none`` n = 0;  1 ``gaussian`` n = a z;  2 ``shot`` n = (a / 8) sqrt(clip((v + 1) / 2, 0, 1)) z -- the Gaussian
    approximation of Poisson noise at 256 levels with Real-ESRGAN's ``poisson_scale`` a.  Colour noise: v is the element and z the
    stream ``expected_noise`` restates; grey noise: v is the pixel's luma (C = 3: BT.601, otherwise the channel mean), one z per
    pixel (``expected_noise(grey=True)``) and the same n in every channel.  ``step`` as in ``degrade``.  n is a constant under
    autograd, for shot noise too: the gradient is ``dy`` where the output lies strictly inside (-1, 1)."""
    require_gpu_tensor(x, 'degrade_noise input')
    if x.dim() != 4 or not 1 <= x.shape[1] <= 4 or x.dtype != torch.float32:
        raise ValueError('degrade_noise: an fp32 [N, C, h, w] batch with 1 to 4 channels is expected, got %s %s' % (x.dtype, tuple(x.shape)))
    x = x.contiguous()
    n = x.shape[0]
    seed, rank = check_seed_rank(seed, rank, 'degrade_noise')
    table = torch.as_tensor(noise_table).to(device=x.device, dtype=torch.float32).contiguous()
    if tuple(table.shape) != (n, 4):
        raise ValueError('degrade_noise: noise_table must be [N = %d, 4], got %s' % (n, tuple(table.shape)))
    return _DegradeNoise.apply(x, table, step_tensor(step, x.device), seed, rank, bool(clamp))


class HighOrderDegrader(DrawStream):
    """The second-order degradation of Real-ESRGAN on the device: every stage draws a blur kernel from seven families, resamples,
    adds Gaussian or shot noise and compresses; the last stage also runs a sinc filter (ringing and overshoot).

    >>> d = HighOrderDegrader(seed=1)                         # the two published stages
    >>> img_lr = d(img_hr, (48, 48))                          # differentiable in img_hr; nothing is read back
    >>> sisr.install(degradation=d)

    Per stage, in this order: ``draw_mix`` (sisr_degrade_draw_mix: ``step`` advances by ONE per stage, so the noise and JPEG-quality
    streams, keyed by the step, are independent between stages), sisr_jpeg_tables on the drawn step if the stage compresses,
    ``degrade(x, size, kernels, None, clamp=False)``, ``degrade_noise(..., clamp=True)``, ``jpeg_roundtrip``.

    ``stages``           ``DegradeStage`` records.  Every stage but the last resamples to the middle size, the last to
                         ``image_size_lr``.
    ``mid_size``         a fixed middle size (h, w): nothing is read back and the call is capturable (graph.GraphedStep).
    ``mid_scale``        (lo, hi): the middle size is the HR size times a factor drawn on the HOST per call from
                         ``numpy.random.default_rng((seed, rank, calls))``; shapes change from call to call, a call under stream
                         capture raises.  Neither given: the rounded geometric mean of the HR and LR sizes.
    ``final_sinc_prob``  the probability that the sample's final filter is a sinc kernel (otherwise the delta kernel); None: no
                         final filter.  The filter is ``degrade`` at equal sizes, where the cubic taps are exactly (0, 1, 0, 0): a pure
                         blur, clamped.  ``final_order``: 'sinc_jpeg' filters before the last stage's JPEG round trip, 'jpeg_sinc' after.
    ``resize_probs``     None: every stage resamples with the align-corners bicubic fused into ``degrade`` (section 18).  A triple of
                         weights (area, bilinear, bicubic): every stage draws a resampler PER SAMPLE on its drawn step
                         (sisr_resize_modes_draw: the count does not advance, ``state_dict`` is unchanged) and becomes
                         ``degrade`` at equal sizes -- a pure blur -- followed by ``resize.resize`` with torch's half-pixel
                         coordinates, Real-ESRGAN's ``random.choice(['area', 'bilinear', 'bicubic'])``; ``last_modes[i]`` [N] int32.
    ``last_*``           the latest call's tables, one entry per stage: ``last_kernels``, ``last_params``, ``last_noise_table``,
                         ``last_drawn_step``, ``last_tables`` / ``last_quality`` (None without JPEG), ``last_sizes``; and
                         ``last_final_kernels``.  ``step``: the 0-dim int64 device tensor of draws made so far."""

    def __init__(self, stages=None, mid_size=None, mid_scale=None, final_sinc_prob=0.8, final_order='sinc_jpeg', seed=0, rank=0,
                 device=None, jpeg_subsampling='420', jpeg_grad='ste', resize_probs=None):
        who = 'HighOrderDegrader'
        self.resize_probs = None
        if resize_probs is not None:
            from .resize import _check_probs
            self.resize_probs = _check_probs(resize_probs, who)
        self.stages = tuple(realesrgan_stages() if stages is None else stages)
        if not self.stages or not all(isinstance(s, DegradeStage) for s in self.stages):
            raise ValueError('%s: stages must be a non-empty sequence of DegradeStage' % who)
        if mid_size is not None and mid_scale is not None:
            raise ValueError('%s: give mid_size or mid_scale, not both' % who)
        self.mid_size = None
        if mid_size is not None:
            self.mid_size = (int(mid_size[0]), int(mid_size[1]))
            if min(self.mid_size) < 1:
                raise ValueError('%s: mid_size must be >= 1, got %s' % (who, self.mid_size))
        self.mid_scale = None if mid_scale is None else _check_range(mid_scale, who, 'mid_scale', True)
        self.final_sinc_prob = None if final_sinc_prob is None else _check_prob(final_sinc_prob, who, 'final_sinc_prob')
        if final_order not in ('sinc_jpeg', 'jpeg_sinc'):
            raise ValueError("%s: final_order is 'sinc_jpeg' or 'jpeg_sinc', got %r" % (who, final_order))
        if jpeg_subsampling not in J.SUBSAMPLING or jpeg_grad not in J.GRAD:
            raise ValueError("%s: jpeg_subsampling is '444' or '420' and jpeg_grad 'ste' or 'cubic', got %r, %r"
                             % (who, jpeg_subsampling, jpeg_grad))
        self.final_order, self.jpeg_subsampling, self.jpeg_grad = final_order, jpeg_subsampling, jpeg_grad
        self._init_stream(seed, rank, device)
        self.calls = 0
        self._mix = [s.c_struct(self.final_sinc_prob if i == len(self.stages) - 1 else None) for i, s in enumerate(self.stages)]
        none = [None] * len(self.stages)
        self.last_kernels, self.last_params, self.last_noise_table, self.last_drawn_step = list(none), list(none), list(none), list(none)
        self.last_tables, self.last_quality, self.last_sizes, self.last_final_kernels = list(none), list(none), list(none), None
        self.last_modes = list(none)

    def draw_mix(self, i, n):
        """the tables of the next step for stage ``i`` and a batch of ``n``: -> (kernels, final_kernels or None, params, noise_table,
        drawn_step) on the device; advances ``step``"""
        dev, K = self.step.device, self.stages[i].ksize
        final = i == len(self.stages) - 1 and self.final_sinc_prob is not None
        k = torch.empty((n, K, K), dtype=torch.float32, device=dev)
        fk = torch.empty((n, K, K), dtype=torch.float32, device=dev) if final else None
        p = torch.empty((n, 8), dtype=torch.float32, device=dev)
        nt = torch.empty((n, 4), dtype=torch.float32, device=dev)
        t = torch.empty((), dtype=torch.int64, device=dev)
        L.check(L.lib().sisr_degrade_draw_mix(self.step.data_ptr(), self.seed, self.rank, n, C.byref(self._mix[i]), k.data_ptr(),
                                              None if fk is None else fk.data_ptr(), p.data_ptr(), nt.data_ptr(), t.data_ptr(),
                                              _stream()), 'sisr_degrade_draw_mix')
        self.last_kernels[i], self.last_params[i], self.last_noise_table[i], self.last_drawn_step[i] = k, p, nt, t
        if final:
            self.last_final_kernels = fk
        return k, fk, p, nt, t

    def stage_sizes(self, size_hr, size_lr):
        """the output size of every stage for this call (``mid_scale``: drawn on the host from the call count)"""
        mid = self.mid_size
        if len(self.stages) > 1 and mid is None:
            if self.mid_scale is not None:
                if torch.cuda.is_current_stream_capturing():
                    raise RuntimeError('HighOrderDegrader: mid_scale draws a new size on the host per call and cannot be captured; '
                                       'give a fixed mid_size')
                s = float(np.random.default_rng((self.seed, self.rank, self.calls)).uniform(*self.mid_scale))
                mid = tuple(max(1, int(round(v * s))) for v in size_hr)
            else:
                mid = tuple(max(1, int(round(math.sqrt(a * b)))) for a, b in zip(size_hr, size_lr))
        return [mid] * (len(self.stages) - 1) + [size_lr]

    def __call__(self, img_hr, image_size_lr):
        require_gpu_tensor(img_hr, 'HighOrderDegrader input')
        if img_hr.device != self.step.device:
            raise RuntimeError('HighOrderDegrader: the batch is on %s, the draws on %s' % (img_hr.device, self.step.device))
        if img_hr.dim() != 4 or img_hr.dtype != torch.float32:
            raise ValueError('HighOrderDegrader: an fp32 [N, C, H, W] batch is expected, got %s %s' % (img_hr.dtype, tuple(img_hr.shape)))
        n = int(img_hr.shape[0])
        size_lr = (int(image_size_lr[0]), int(image_size_lr[1]))
        sizes = self.stage_sizes((int(img_hr.shape[2]), int(img_hr.shape[3])), size_lr)
        self.calls += 1
        x = img_hr
        for i, st in enumerate(self.stages):
            k, fk, _, nt, t = self.draw_mix(i, n)
            # before the forward: the draws of a step stay together
            q, tables = (None, None) if st.jpeg is None else J.draw_tables(t, self.seed, self.rank, n, *st.jpeg)
            self.last_quality[i], self.last_tables[i], self.last_sizes[i] = q, tables, sizes[i]
            if self.resize_probs is None:
                x = degrade(x, sizes[i], k, None, clamp=False)
            else:                                                         # a pure blur at the stage's input size, then the drawn resampler
                from .resize import draw_resize_modes, resize
                modes = self.last_modes[i] = draw_resize_modes(t, self.seed, self.rank, n, self.resize_probs)
                x = degrade(x, (int(x.shape[2]), int(x.shape[3])), k, None, clamp=False)
                x = resize(x, sizes[i], modes)
            x = degrade_noise(x, nt, t, self.seed, self.rank, clamp=True)
            if fk is not None and self.final_order == 'sinc_jpeg':
                x = degrade(x, sizes[i], fk, None, clamp=True)
            if tables is not None:
                x = J.jpeg_roundtrip(x, tables, self.jpeg_subsampling, self.jpeg_grad, True)
            if fk is not None and self.final_order == 'jpeg_sinc':
                x = degrade(x, sizes[i], fk, None, clamp=True)
        return x

    lr_from_hr = Degrader.lr_from_hr                                       # the same adapter to the reference's signature

    def state_dict(self):
        return dict(super().state_dict(), calls=self.calls)

    def load_state_dict(self, state):
        super().load_state_dict(state)
        self.calls = int(state.get('calls', 0))
