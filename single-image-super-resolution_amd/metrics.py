"""Image-quality metrics on the device: per-image PSNR and SSIM of two NCHW batches on the gfx950 kernels of
csrc/metrics.hip, and ``evaluate_generator`` -- a whole validation pass (degrade, super-resolve in eval mode, score).

The reference reports neither number (its to-do list, README.md:88); a host-side SSIM would need a device -> host copy in
the middle of the training loop.  Here nothing synchronises with the host: the results are fp32 device tensors, bit-identical
from call to call, and the launches can be captured by ``graph.GraphedStep``.

These are METRICS, not losses: the inputs are detached and nothing here is differentiable.

Definitions (sisr_hip.h): the view ``crop_border`` (pixels stripped from every side) and ``luma`` (C == 3: the BT.601
full-range plane Y = 0.299 R + 0.587 G + 0.114 B of the normalised values) is applied first;
PSNR = 10 log10(data_range^2 / mse), +inf for equal images; SSIM is Wang et al.'s with the 11 x 11 Gaussian window
(sigma 1.5), "valid" window positions only, C1 = (0.01 data_range)^2, C2 = (0.03 data_range)^2, averaged over planes and
positions.  ``data_range`` defaults to 2.0: the project's images are normalised to [-1, 1].
``ms_ssim`` (csrc/ms_ssim.hip) is the multi-scale form with ``len(weights)`` scales; ``check_ms_ssim`` / ``ms_ssim_forward`` are
shared with ``losses.ms_ssim_loss``, its differentiable counterpart.
``niqe`` (csrc/niqe.hip) is the one NO-REFERENCE score: it needs a ``NiqeModel`` -- loaded from an ``.npz`` or
fitted on the user's own sharp images with ``NiqeModel.fit`` -- and no ground truth.
"""
import contextlib
import ctypes
import math

import numpy as np
import torch

from . import _lib as L
from .engine import _stream, require_gpu_tensor
from .utils import lr_from_hr

WINDOW = 11
MS_SSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)      # Wang, Simoncelli, Bovik 2003: five scales, finest first
MS_SSIM_MAX_SCALES = 5


def check_view(a, b, data_range, crop_border, least=WINDOW, what='metrics'):
    """The view rule of the metrics and of ``losses.image_loss``, stated once: two 4-D [N, C, H, W] tensors of one shape, C 1 or
    3, ``crop_border`` a non-negative integer (no bool) that leaves ``least`` x ``least`` pixels (the SSIM window; 1 for a pixel
    term alone), ``data_range`` > 0.  -> crop_border as an int.  Argument errors come before the device check: they are the
    caller's, whatever the tensors live on"""
    for t in (a, b):
        if not isinstance(t, torch.Tensor) or t.dim() != 4:
            raise ValueError('%s: two 4-D [N, C, H, W] tensors are expected, got %s'
                             % (what, tuple(t.shape) if isinstance(t, torch.Tensor) else type(t)))
    if a.shape != b.shape:
        raise ValueError('%s: the images differ in shape: %s vs %s' % (what, tuple(a.shape), tuple(b.shape)))
    n, c, h, w = a.shape
    if n < 1:
        raise ValueError('%s: empty batch' % what)
    if c not in (1, 3):
        raise ValueError('%s: 1 or 3 channels expected, got %d' % (what, c))
    if not float(data_range) > 0.0:
        raise ValueError('%s: data_range must be positive, got %r' % (what, data_range))
    if isinstance(crop_border, bool) or crop_border != int(crop_border) or crop_border < 0:
        raise ValueError('%s: crop_border must be a non-negative integer, got %r' % (what, crop_border))
    crop = int(crop_border)
    if h - 2 * crop < least or w - 2 * crop < least:
        raise ValueError('%s: %d x %d pixels remain after cropping %d from every side; %d x %d are needed'
                         % (what, h - 2 * crop, w - 2 * crop, crop, least, least))
    return crop


def _native(t, what):
    """the kernels' form: detached fp32 contiguous device tensor"""
    t = t.detach().float()
    require_gpu_tensor(t, what)
    return t.contiguous()


def _run(a, b, data_range, crop_border, luma, want_psnr, want_ssim):
    crop = check_view(a, b, data_range, crop_border)
    a, b = _native(a, 'metrics input a'), _native(b, 'metrics input b')
    if a.device != b.device:
        raise ValueError('metrics: the images live on different devices: %s vs %s' % (a.device, b.device))
    n, c, h, w = a.shape
    lib = L.lib()
    ws = L.check_count(lib.sisr_image_metrics_ws_floats(n, c, h, w, crop, int(bool(luma))), 'sisr_image_metrics_ws_floats')
    work = torch.empty(ws, dtype=torch.float32, device=a.device)
    psnr_t = torch.empty(n, dtype=torch.float32, device=a.device) if want_psnr else None
    ssim_t = torch.empty(n, dtype=torch.float32, device=a.device) if want_ssim else None
    L.check(lib.sisr_image_metrics(a.data_ptr(), b.data_ptr(), n, c, h, w, crop, int(bool(luma)), float(data_range),
                                   work.data_ptr(), None if psnr_t is None else psnr_t.data_ptr(),
                                   None if ssim_t is None else ssim_t.data_ptr(), _stream()), 'sisr_image_metrics')
    return psnr_t, ssim_t


def psnr(a, b, data_range=2.0, crop_border=0, luma=False):
    """per-image peak signal-to-noise ratio in dB -> fp32 Tensor[N] on the inputs' device (a metric: inputs are detached)"""
    return _run(a, b, data_range, crop_border, luma, True, False)[0]


def ssim(a, b, data_range=2.0, crop_border=0, luma=False):
    """per-image structural similarity -> fp32 Tensor[N] on the inputs' device (a metric: inputs are detached)"""
    return _run(a, b, data_range, crop_border, luma, False, True)[1]


def psnr_ssim(a, b, data_range=2.0, crop_border=0, luma=False):
    """-> (psnr Tensor[N], ssim Tensor[N]) from one launch sequence (a metric: inputs are detached)"""
    return _run(a, b, data_range, crop_border, luma, True, True)


def check_ms_ssim(a, b, data_range, crop_border, weights, what='ms_ssim'):
    """The argument rule of ``ms_ssim`` and of ``losses.ms_ssim_loss``, stated once: ``check_view``'s, fp32 tensors on one device, a
    finite ``data_range``, 1 to 5 positive finite ``weights`` (one per scale), and a view of at least ``11 << (M - 1)`` pixels a
    side for M scales.  -> (crop_border as an int, the weights as a tuple of floats).  All of it comes before the device check"""
    crop = check_view(a, b, data_range, crop_border, what=what)
    for t in (a, b):
        if t.dtype != torch.float32:
            raise ValueError('%s: fp32 expected, got %s' % (what, t.dtype))
    if a.device != b.device:
        raise ValueError('%s: the images live on different devices: %s vs %s' % (what, a.device, b.device))
    if not math.isfinite(float(data_range)):
        raise ValueError('%s: data_range must be finite, got %r' % (what, data_range))
    try:
        wts = tuple(float(x) for x in weights)
    except TypeError:
        raise ValueError('%s: weights is a sequence of 1 to %d numbers, got %r' % (what, MS_SSIM_MAX_SCALES, weights)) from None
    if not 1 <= len(wts) <= MS_SSIM_MAX_SCALES:
        raise ValueError('%s: 1 to %d weights (one per scale) are expected, got %d' % (what, MS_SSIM_MAX_SCALES, len(wts)))
    for x in wts:
        if not (x > 0.0 and math.isfinite(x)):
            raise ValueError('%s: every weight must be positive and finite, got %r' % (what, wts))
    side = min(a.shape[2], a.shape[3]) - 2 * crop
    fits = max(m for m in range(1, MS_SSIM_MAX_SCALES + 1) if side >> (m - 1) >= WINDOW)
    if len(wts) > fits:
        raise ValueError('%s: %d scales need %d pixels a side, %d x %d remain after cropping %d from every side: at most %d scales fit'
                         % (what, len(wts), WINDOW << (len(wts) - 1), a.shape[2] - 2 * crop, a.shape[3] - 2 * crop, crop, fits))
    return crop, wts


def ms_ssim_forward(a, b, cfg):
    """The forward launches of csrc/ms_ssim.hip on detached contiguous fp32 device tensors; ``cfg`` = (N, C, H, W, crop, luma,
    data_range, weights).  -> (ms [N], terms [M, N, C'], pyr_a, pyr_b): the pyramid buffers hold levels >= 1 of the two inputs"""
    n, c, h, w, crop, luma, data_range, wts = cfg
    lib, dev, m = L.lib(), a.device, len(wts)

    def floats(which):
        return L.check_count(lib.sisr_ms_ssim_ws_floats(n, c, h, w, crop, luma, m, which), 'sisr_ms_ssim_ws_floats')
    pyr_a, pyr_b = (torch.empty(floats(0), dtype=torch.float32, device=dev) for _ in range(2))
    part = torch.empty(floats(1), dtype=torch.float32, device=dev)
    terms = torch.empty((m, n, 1 if (luma and c == 3) else c), dtype=torch.float32, device=dev)
    ms = torch.empty(n, dtype=torch.float32, device=dev)
    L.check(lib.sisr_ms_ssim_fwd(a.data_ptr(), b.data_ptr(), n, c, h, w, crop, luma, data_range, m, weights5(wts), pyr_a.data_ptr(),
                                 pyr_b.data_ptr(), part.data_ptr(), terms.data_ptr(), ms.data_ptr(), _stream()), 'sisr_ms_ssim_fwd')
    return ms, terms, pyr_a, pyr_b


def weights5(wts):
    """the host array of five floats that the entry points of csrc/ms_ssim.hip take"""
    return (ctypes.c_float * MS_SSIM_MAX_SCALES)(*(tuple(wts) + (0.0,) * (MS_SSIM_MAX_SCALES - len(wts))))


def ms_ssim(a, b, data_range=2.0, crop_border=0, luma=False, weights=MS_SSIM_WEIGHTS, return_terms=False):
    """per-image multi-scale SSIM (Wang, Simoncelli, Bovik 2003) -> fp32 Tensor[N] on the inputs' device (a metric: inputs are
    detached); with ``return_terms`` also ``terms [M, N, C']``.  M = ``len(weights)`` scales, ``weights`` used as given (not
    renormalised): the view (``crop_border``, ``luma``) is applied once, every further scale is the 2 x 2 mean of the one before
    (an odd last row / column is dropped), and with ``cs`` the contrast-structure factor and ``l`` the luminance factor of the
    SSIM map, ``terms[j]`` is the mean of ``cs`` for j < M - 1 and of ``l cs`` (SSIM) for the last scale.  Per image and plane the
    score is ``prod_j terms[j] ** weights[j]``, exactly 0 when a term is <= 0; the planes are averaged.  The view needs
    ``11 << (M - 1)`` pixels a side (176 for the default five scales).  fp32 inputs; non-contiguous ones are made contiguous"""
    crop, wts = check_ms_ssim(a, b, data_range, crop_border, weights)
    a, b = _native(a, 'ms_ssim input a'), _native(b, 'ms_ssim input b')
    n, c, h, w = a.shape
    ms, terms, _, _ = ms_ssim_forward(a, b, (n, c, h, w, crop, int(bool(luma)), float(data_range), wts))
    return (ms, terms) if return_terms else ms


# ---- NIQE: the no-reference score (csrc/niqe.hip; the definition is stated in sisr_hip.h and DESIGN.md section 30) ---------------------
NIQE_FEATURES = L.NIQE_FEATURES
_NIQE_TABLES = {}


def niqe_tables_host():
    """float64 [4, 9801]: Gamma(1 / a_j), Gamma(2 / a_j), Gamma(3 / a_j) by ``math.gamma`` and rho_j = G2^2 / (G1 G3) formed from them,
    a_j = 0.2 + 0.001 j: what the AGGD fit searches (host code, no GPU)"""
    a = 0.2 + 0.001 * np.arange(L.NIQE_TABLE, dtype=np.float64)
    g = np.array([[math.gamma(k / float(x)) for x in a] for k in (1.0, 2.0, 3.0)], dtype=np.float64)
    return np.concatenate([g, (g[1] * g[1] / (g[0] * g[2]))[None]], axis=0)


def _niqe_tables(device):
    """the tables on ``device``, built and uploaded once per device (call once before capturing a graph)"""
    key = str(device)
    if key not in _NIQE_TABLES:
        _NIQE_TABLES[key] = torch.from_numpy(niqe_tables_host()).to(device)
    return _NIQE_TABLES[key]


def check_niqe(img, block, crop_border, value_range, what='niqe'):
    """The argument rule of ``niqe_features`` / ``niqe`` / ``NiqeModel.fit``, before the device check as in ``check_view``: a 4-D fp32
    [N, C, H, W] tensor, C 1 or 3, an even ``block`` in 16 .. 96, a non-negative integer ``crop_border`` that leaves one block, a
    finite ``value_range = (lo, hi)`` with lo < hi.  -> (block, crop, lo, hi)"""
    if not isinstance(img, torch.Tensor) or img.dim() != 4:
        raise ValueError('%s: a 4-D [N, C, H, W] tensor is expected, got %s'
                         % (what, tuple(img.shape) if isinstance(img, torch.Tensor) else type(img)))
    if img.dtype != torch.float32:
        raise ValueError('%s: fp32 expected, got %s' % (what, img.dtype))
    n, c, h, w = img.shape
    if n < 1:
        raise ValueError('%s: empty batch' % what)
    if c not in (1, 3):
        raise ValueError('%s: 1 or 3 channels expected, got %d' % (what, c))
    if isinstance(block, bool) or not isinstance(block, int) or block % 2 or not 16 <= block <= L.NIQE_MAX_BLOCK:
        raise ValueError('%s: block must be an even integer in 16 .. %d, got %r' % (what, L.NIQE_MAX_BLOCK, block))
    if isinstance(crop_border, bool) or not isinstance(crop_border, int) or crop_border < 0:
        raise ValueError('%s: crop_border must be a non-negative integer, got %r' % (what, crop_border))
    try:
        lo, hi = (float(v) for v in value_range)
    except (TypeError, ValueError):
        raise ValueError('%s: value_range is a pair (lo, hi), got %r' % (what, value_range)) from None
    if not (math.isfinite(lo) and math.isfinite(hi) and lo < hi):
        raise ValueError('%s: value_range must be finite with lo < hi, got %r' % (what, value_range))
    if h - 2 * crop_border < block or w - 2 * crop_border < block:
        raise ValueError('%s: %d x %d pixels remain after cropping %d from every side; one %d x %d block is needed'
                         % (what, h - 2 * crop_border, w - 2 * crop_border, crop_border, block, block))
    return block, crop_border, lo, hi


def _niqe_features(img, block, crop, lo, hi, want_sharp):
    """the four launches of sisr_niqe_features on a detached contiguous fp32 device tensor -> (feat [N, nb, 36] float64, sharp or
    None, the workspace)"""
    n, c, h, w = img.shape
    lib, dev = L.lib(), img.device
    nb = ((h - 2 * crop) // block) * ((w - 2 * crop) // block)
    ws = torch.empty(L.check_count(lib.sisr_niqe_ws_bytes(n, h, w, crop, block), 'sisr_niqe_ws_bytes') // 8, dtype=torch.float64, device=dev)
    feat = torch.empty((n, nb, NIQE_FEATURES), dtype=torch.float64, device=dev)
    sharp = torch.empty((n, nb), dtype=torch.float32, device=dev) if want_sharp else None
    L.check(lib.sisr_niqe_features(img.data_ptr(), n, c, h, w, crop, lo, hi, block, _niqe_tables(dev).data_ptr(), ws.data_ptr(),
                                   feat.data_ptr(), None if sharp is None else sharp.data_ptr(), _stream()), 'sisr_niqe_features')
    return feat, sharp, ws


def niqe_features(img, block=96, crop_border=0, value_range=(-1.0, 1.0), return_sharpness=False):
    """The 36 NIQE features of every ``block`` x ``block`` block of the luma plane (18 per scale, scale 1 first; blocks row-major over
    the top-left whole blocks of the cropped view) -> float64 ``[N, nb, 36]`` on the input's device; with ``return_sharpness`` also
    the blocks' mean local deviation at scale 1, fp32 ``[N, nb]`` (what ``NiqeModel.fit`` selects by).  A fit with an empty side
    (a constant block) has alpha = 0.2 and NaNs elsewhere.  A metric: the input is detached."""
    block, crop, lo, hi = check_niqe(img, block, crop_border, value_range, 'niqe_features')
    feat, sharp, _ = _niqe_features(_native(img, 'niqe_features input'), block, crop, lo, hi, bool(return_sharpness))
    return (feat, sharp) if return_sharpness else feat


class NiqeModel:
    """The "pristine" model of NIQE: the mean ``mu`` [36] and the covariance ``cov`` [36, 36] of the features over sharp blocks of good
    images, and the ``block`` size they were taken at (float64 tensors).  Scores under different models are not comparable."""

    def __init__(self, mu, cov, block=96):
        mu = torch.as_tensor(mu, dtype=torch.float64).detach()
        cov = torch.as_tensor(cov, dtype=torch.float64).detach()
        if mu.dim() == 2 and mu.shape[0] == 1:
            mu = mu[0]
        if tuple(mu.shape) != (NIQE_FEATURES,) or tuple(cov.shape) != (NIQE_FEATURES, NIQE_FEATURES):
            raise ValueError('NiqeModel: mu [36] (or [1, 36]) and cov [36, 36] are expected, got %s and %s' % (tuple(mu.shape), tuple(cov.shape)))
        if isinstance(block, bool) or not isinstance(block, (int, np.integer)) or block % 2 or not 16 <= block <= L.NIQE_MAX_BLOCK:
            raise ValueError('NiqeModel: block must be an even integer in 16 .. %d, got %r' % (L.NIQE_MAX_BLOCK, block))
        if cov.device != mu.device:
            raise ValueError('NiqeModel: mu and cov live on different devices: %s vs %s' % (mu.device, cov.device))
        self.mu, self.cov, self.block = mu.contiguous(), cov.contiguous(), int(block)

    def to(self, device):
        return NiqeModel(self.mu.to(device), self.cov.to(device), self.block)

    def save(self, path):
        """an ``.npz`` with BasicSR's names: ``mu_pris_param`` [1, 36], ``cov_pris_param`` [36, 36], and ``block``"""
        with open(path, 'wb') as f:
            np.savez(f, mu_pris_param=self.mu.cpu().numpy()[None], cov_pris_param=self.cov.cpu().numpy(), block=np.int64(self.block))

    @classmethod
    def load(cls, path):
        """reads ``save``'s file, or a BasicSR-style parameter file (no ``block`` entry: 96) -> a model on the CPU"""
        with np.load(path) as z:
            if 'mu_pris_param' not in z.files or 'cov_pris_param' not in z.files:
                raise ValueError("NiqeModel.load: %s holds no 'mu_pris_param' / 'cov_pris_param' (it has %s)" % (path, z.files))
            return cls(z['mu_pris_param'].astype(np.float64), z['cov_pris_param'].astype(np.float64),
                       int(z['block']) if 'block' in z.files else 96)

    @classmethod
    def fit(cls, batches, block=96, sharpness=0.75, crop_border=0, value_range=(-1.0, 1.0)):
        """Fit a model as the paper does: over ``batches`` (an iterable of fp32 [N, C, H, W] device tensors, of any sizes) keep the
        feature rows of the blocks whose sharpness exceeds ``sharpness`` times the largest of their own image, drop rows with a NaN,
        and take the mean and the unbiased covariance of what is left.  The features come from the kernels; selection and moments
        are torch ops and the call synchronises: an offline step.  Fewer than 37 kept rows is an error."""
        if not (isinstance(sharpness, (int, float)) and not isinstance(sharpness, bool) and 0.0 <= float(sharpness) < 1.0):
            raise ValueError('NiqeModel.fit: sharpness must lie in [0, 1), got %r' % (sharpness,))
        rows = []
        for img in batches:
            feat, sharp = niqe_features(img, block, crop_border, value_range, return_sharpness=True)
            keep = sharp > float(sharpness) * sharp.amax(dim=1, keepdim=True)
            keep &= ~torch.isnan(feat).any(dim=2)
            rows.append(feat[keep])
        if not rows:
            raise ValueError('NiqeModel.fit: no images')
        rows = torch.cat(rows)
        if rows.shape[0] <= NIQE_FEATURES:
            raise ValueError('NiqeModel.fit: %d feature rows were kept, at least %d are needed for a covariance of full rank'
                             % (rows.shape[0], NIQE_FEATURES + 1))
        mu = rows.mean(dim=0)
        dev = rows - mu
        return cls(mu, dev.t() @ dev / (rows.shape[0] - 1), block)


def niqe(img, model, crop_border=0, value_range=(-1.0, 1.0)):
    """per-image NIQE of ``img`` under ``model`` (a ``NiqeModel`` on the image's device; lower is better) -> fp32 Tensor[N].  No
    reference image is needed.  Five launches whatever N is, nothing read back, capturable once a first call has uploaded the
    tables; fewer than two NaN-free blocks or a (cov_p + cov_d) that is not positive definite gives NaN.  A metric: the input is detached."""
    if not isinstance(model, NiqeModel):
        raise ValueError('niqe: model must be a NiqeModel, got %s' % type(model))
    block, crop, lo, hi = check_niqe(img, model.block, crop_border, value_range)
    img = _native(img, 'niqe input')
    if model.mu.device != img.device:
        raise ValueError('niqe: the model lives on %s, the image on %s (NiqeModel.to)' % (model.mu.device, img.device))
    feat, _, ws = _niqe_features(img, block, crop, lo, hi, False)
    score = torch.empty(img.shape[0], dtype=torch.float32, device=img.device)
    L.check(L.lib().sisr_niqe_score(feat.data_ptr(), feat.shape[0], feat.shape[1], model.mu.data_ptr(), model.cov.data_ptr(),
                                    ws.data_ptr(), score.data_ptr(), _stream()), 'sisr_niqe_score')
    return score


def evaluate_generator(net_g, img_hr, image_size_lr, crop_border=None, luma=False, ema=None, niqe_model=None):
    """One validation pass: ``lr_from_hr(img_hr)`` -> ``net_g`` in eval mode under ``no_grad`` -> ``psnr_ssim(sr, img_hr)``.

    Eval mode means running-statistics BatchNorm and no spectral-norm power iteration, so -- unlike calling the net in train
    mode, as the reference's ``save_curr_vis`` does -- the pass leaves every buffer of ``net_g`` as it was (BatchNorm running
    statistics, ``num_batches_tracked``, spectral-norm ``u`` / ``v``).  The training flag of every submodule is restored
    afterwards, also when the pass raises.  ``crop_border=None`` crops by the scale factor (the SR convention).
    ``ema`` (an ``ema.WeightEMA`` over ``net_g``): the forward runs inside ``ema.applied()`` -- the AVERAGED weights are scored
    and the live ones are back in place, bit for bit, afterwards.
    ``niqe_model`` (a ``NiqeModel``): the dict gains ``niqe``, the no-reference score of the SR batch under that model, cropped by the
    same border; without one the dict and every launch are as they were.
    Returns ``dict(psnr=Tensor[N], ssim=Tensor[N])``."""
    if ema is not None and ema.module is not net_g:
        raise ValueError('evaluate_generator: ema averages another module than net_g')
    modes = [(m, m.training) for m in net_g.modules()]
    with contextlib.nullcontext() if ema is None else ema.applied():
        try:
            net_g.eval()
            with torch.no_grad():
                lr = lr_from_hr(img_hr, image_size_lr)
                sr = net_g(lr)
        finally:
            for m, was in modes:
                m.training = was
    if sr.shape != img_hr.shape:
        raise ValueError('evaluate_generator: the generator maps %s to %s, the HR batch is %s'
                         % (tuple(lr.shape), tuple(sr.shape), tuple(img_hr.shape)))
    if crop_border is None:
        crop_border = sr.shape[-1] // lr.shape[-1]
    p, s = psnr_ssim(sr, img_hr, crop_border=crop_border, luma=luma)
    if niqe_model is None:
        return dict(psnr=p, ssim=s)
    return dict(psnr=p, ssim=s, niqe=niqe(sr.float(), niqe_model, crop_border=crop_border))
