"""The losses of an SRGAN iteration on the device: the feature ("content") MSE of train.py:183-186 and the binary cross-entropy
of config.py:107 as fused gfx950 kernels (csrc/losses.hip), forward and backward, and the three loss functions of
train.py:128-186 written on top of them with their globals made arguments.

The torch expressions they stand in for, ``torch.mean(torch.pow(a - b, 2))`` and ``nn.BCELoss()(p, label)``, are elementwise
launches: the MSE moves its two feature tensors (70.8 MB each at B16 / HR 96^2 under ``MaskedVGG(0b01111)``) through HBM at least
11 times forward + backward and keeps ``a - b`` alive; ``feature_mse`` takes 5 passes (read a and b, read them again, write one
gradient) and saves nothing but its inputs.  ``bce_loss`` needs no label tensor, returns mean(p) -- the ``D_x`` / ``D_G_z``
statistics -- from the same launch, and has no device-side range assertion: a NaN in gives a NaN out, never an abort.

``image_loss`` (csrc/image_loss.hip) is the image-space term that SR trainers put beside those two: ``ssim_weight * (1 - SSIM) +
pixel_weight * mean(rho(a - b))`` with rho L1, Charbonnier or MSE, on the crop / luma view and with the SSIM of ``metrics``; two
launches forward, one backward, nothing saved but the inputs (the torch-op composition of SSIM alone is ten ``conv2d`` and about
thirty elementwise launches with some fifteen saved image-size intermediates).  ``ssim_loss``, ``l1_loss`` and
``charbonnier_loss`` are its one-term forms.

``ms_ssim_loss`` (csrc/ms_ssim.hip) is ``1 - MS-SSIM`` with the multi-scale SSIM of ``metrics.ms_ssim``: ``len(weights)`` scales,
one launch per scale and a finish forward, one launch per scale backward; saved are the inputs, their pooled levels and the
per-scale terms.

``frequency_loss`` (csrc/freq_loss.hip) is the frequency-domain term: the FFT-L1 / Charbonnier loss over the half spectrum or the
focal frequency loss, from ONE direct separable DFT of ``a - b`` (view sides up to 256, any length); three launches forward, two
backward; saved are the spectrum and the plane maxima, not the inputs.  ``fft_l1_loss`` and ``focal_frequency_loss`` are its
one-term forms.

``artifact_loss`` (csrc/artifact.hip) is the artifact-aware (locally discriminative, LDL) term of Liang et al., "Details or
Artifacts" (CVPR 2022): an L1 between ``sr`` and ``gt`` weighted by the refined artifact map, which compares the residual of the
generator's output with that of its EMA twin's; ``artifact_map`` is the map alone.  Three launches forward, one backward; saved are
``sr``, ``gt`` and the one-channel map.  The map is a constant of the loss (detached).

``perceptual_loss`` (csrc/percep.hip) is the multi-tap perceptual loss of the ESRGAN / Real-ESRGAN recipes (BasicSR's
``PerceptualLoss``): a per-tap L1 / L2 / Frobenius criterion over the taps of a ``MaskedVGG`` feature vector with one weight per tap,
and the optional style term on the Gram matrices of the same taps, which run on the exact-fp32 matrix instruction.  Four launches
forward with both terms, one backward; saved are the inputs, the derivative ``D`` of the style term with respect to the Gram
matrices and the per-tap terms.  ``gram_matrix`` is the Gram matrices alone; ``PerceptualLoss`` the module around an extractor.

``contextual_loss`` (csrc/contextual.hip) is the contextual loss of Mechrez et al. (ECCV 2018) in its cosine form over the same taps: it
compares every feature point of the generator's side with every point of the target's, so it matches the distribution of the
target's features, not each position's.  The ``P x P`` similarity runs on the exact-fp32 matrix instruction and lives in a workspace;
six launches forward, four backward; saved are the inputs and ``O(B P)`` tables.  ``contextual_similarity`` is the similarity alone;
``ContextualLoss`` the module around an extractor.

Nothing here synchronises with the host: losses and statistics are 0-dim fp32 device tensors, bit-identical from call to call,
and the launches can be captured by ``graph.GraphedStep``.  Opt-in: ``install(fused_losses=True)`` points ``torch.nn.BCELoss`` at
``BCELoss``; a trainer rebinds its ``content_loss_g`` / ``adversarial_loss_*`` to the functions below.
"""
import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _lib as L
from .engine import _stream, require_gpu_tensor
from .metrics import MS_SSIM_WEIGHTS, WINDOW, check_ms_ssim, check_view, ms_ssim_forward, weights5


def _check_tensor(t, what):
    if not isinstance(t, torch.Tensor):
        raise ValueError('%s: a tensor is expected, got %s' % (what, type(t)))
    if t.dtype != torch.float32:
        raise ValueError('%s: fp32 expected, got %s' % (what, t.dtype))
    if t.numel() < 1:
        raise ValueError('%s: empty tensor' % what)


def _validate_pair(a, b, what):
    """argument errors come before the device check: they are the caller's, whatever the tensors live on"""
    _check_tensor(a, what)
    _check_tensor(b, what)
    if a.shape != b.shape:
        raise ValueError('%s: the tensors differ in shape (no broadcasting): %s vs %s' % (what, tuple(a.shape), tuple(b.shape)))
    if a.device != b.device:
        raise ValueError('%s: the tensors live on different devices: %s vs %s' % (what, a.device, b.device))


def _scalar(dev):
    return torch.empty((), dtype=torch.float32, device=dev)


def _check_reduction(reduction, what):
    if reduction not in ('mean', 'none'):
        raise ValueError("%s: reduction is 'mean' or 'none', got %r" % (what, reduction))


def _ptr(t):
    """the device address of an optional tensor, None (a null pointer) without one"""
    return None if t is None else t.data_ptr()


def _wanted_grads(ctx, shape, dev):
    """(da, db): an uninitialised fp32 gradient for each of the first two inputs that needs one, else None"""
    return tuple(torch.empty(shape, dtype=torch.float32, device=dev) if need else None for need in ctx.needs_input_grad[:2])


class _FeatureMSE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, weight):
        a, b = a.detach().contiguous(), b.detach().contiguous()
        lib, n = L.lib(), a.numel()
        work = torch.empty(L.check_count(lib.sisr_mse_ws_floats(n), 'sisr_mse_ws_floats'), dtype=torch.float32, device=a.device)
        loss = _scalar(a.device)
        L.check(lib.sisr_mse_fwd(a.data_ptr(), b.data_ptr(), n, weight, work.data_ptr(), loss.data_ptr(), _stream()),
                'sisr_mse_fwd')
        ctx.save_for_backward(a, b)            # the inputs themselves (their contiguous form): no intermediate is kept
        ctx.weight = weight
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        g = g.to(torch.float32).contiguous()
        da, db = _wanted_grads(ctx, a.shape, a.device)
        if da is not None or db is not None:
            L.check(L.lib().sisr_mse_bwd(a.data_ptr(), b.data_ptr(), g.data_ptr(), a.numel(), ctx.weight,
                                         _ptr(da), _ptr(db), _stream()), 'sisr_mse_bwd')
        return da, db, None


def feature_mse(a, b, weight=1.0):
    """``weight * torch.mean(torch.pow(a - b, 2))`` -> 0-dim fp32 device tensor; differentiable with respect to ``a``, ``b`` or
    both (only what requires a gradient is computed).  Any two equal shapes: feature maps, or images under the ``identity()``
    extractor.  Non-contiguous inputs are made contiguous first."""
    _validate_pair(a, b, 'feature_mse')
    require_gpu_tensor(a, 'feature_mse input a')
    require_gpu_tensor(b, 'feature_mse input b')
    return _FeatureMSE.apply(a, b, float(weight))


PIXEL_KINDS = {'l1': L.PIX_L1, 'charbonnier': L.PIX_CHARBONNIER, 'mse': L.PIX_MSE}


class _ImageLoss(torch.autograd.Function):
    """-> (loss[N], ssim[N] or None, pix[N] or None); ``cfg`` = (N, C, H, W, crop, luma, data_range, w_ssim, w_pix, kind, eps)"""

    @staticmethod
    def forward(ctx, a, b, cfg, want_parts):
        a, b = a.detach().contiguous(), b.detach().contiguous()
        n, c, h, w, crop, luma, data_range, w_ssim, w_pix, kind, eps = cfg
        lib, dev = L.lib(), a.device
        with_ssim = int(w_ssim != 0.0 or want_parts)
        ws = L.check_count(lib.sisr_image_loss_ws_floats(n, c, h, w, crop, luma, with_ssim), 'sisr_image_loss_ws_floats')
        work = torch.empty(ws, dtype=torch.float32, device=dev)
        loss = torch.empty(n, dtype=torch.float32, device=dev)
        ssim = torch.empty(n, dtype=torch.float32, device=dev) if want_parts else None
        pix = torch.empty(n, dtype=torch.float32, device=dev) if want_parts else None
        L.check(lib.sisr_image_loss_fwd(a.data_ptr(), b.data_ptr(), n, c, h, w, crop, luma, data_range, w_ssim, w_pix, kind, eps,
                                        work.data_ptr(), loss.data_ptr(), _ptr(ssim), _ptr(pix), _stream()), 'sisr_image_loss_fwd')
        ctx.save_for_backward(a, b)            # the inputs themselves: the backward recomputes the window moments
        ctx.cfg = cfg
        if want_parts:
            ctx.mark_non_differentiable(ssim, pix)
        return loss, ssim, pix

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _g_ssim, _g_pix):
        a, b = ctx.saved_tensors
        n, c, h, w, crop, luma, data_range, w_ssim, w_pix, kind, eps = ctx.cfg
        da, db = _wanted_grads(ctx, a.shape, a.device)
        if da is not None or db is not None:
            g = g.to(torch.float32).contiguous()
            L.check(L.lib().sisr_image_loss_bwd(a.data_ptr(), b.data_ptr(), g.data_ptr(), n, c, h, w, crop, luma, data_range,
                                                w_ssim, w_pix, kind, eps, _ptr(da), _ptr(db), _stream()), 'sisr_image_loss_bwd')
        return da, db, None, None


def image_loss(a, b, ssim_weight=0.0, pixel_weight=1.0, pixel='l1', eps=1e-3, data_range=2.0, crop_border=0, luma=False,
               reduction='mean', return_parts=False):
    """``ssim_weight * (1 - SSIM[n]) + pixel_weight * mean(rho(a - b))`` per image of two fp32 [N, C, H, W] batches, C 1 or 3, on
    the view of ``metrics`` (``crop_border`` pixels stripped from every side, then the BT.601 plane with ``luma``); SSIM is
    ``metrics.ssim``'s, rho is ``|d|`` ('l1'), ``sqrt(d^2 + eps^2)`` ('charbonnier') or ``d^2`` ('mse').  -> 0-dim fp32 device
    tensor (the mean over the batch), or [N] with ``reduction='none'``; with ``return_parts`` also the detached ``ssim[N]`` and
    ``pix[N]`` (the SSIM passes then run whatever ``ssim_weight`` is).  Differentiable with respect to ``a``, ``b`` or both (only
    what requires a gradient is computed; pixels of the cropped border get exact zeros), once.  The view needs 11 x 11 pixels
    when SSIM is computed, 1 x 1 otherwise.  Non-contiguous inputs are made contiguous first; a bf16 caller casts."""
    what = 'image_loss'
    _validate_pair(a, b, what)
    w_ssim, w_pix = float(ssim_weight), float(pixel_weight)
    crop = check_view(a, b, data_range, crop_border, least=WINDOW if (w_ssim != 0.0 or return_parts) else 1, what=what)
    n, c, h, w = a.shape
    if pixel not in PIXEL_KINDS:
        raise ValueError('%s: pixel is one of %s, got %r' % (what, sorted(PIXEL_KINDS), pixel))
    _check_reduction(reduction, what)
    if not float(eps) >= 0.0:
        raise ValueError('%s: eps must not be negative, got %r' % (what, eps))
    require_gpu_tensor(a, 'image_loss input a')
    require_gpu_tensor(b, 'image_loss input b')
    cfg = (n, c, h, w, crop, int(bool(luma)), float(data_range), w_ssim, w_pix, PIXEL_KINDS[pixel], float(eps))
    loss, ssim, pix = _ImageLoss.apply(a, b, cfg, bool(return_parts))
    if reduction == 'mean':
        loss = loss.mean()
    return (loss, ssim, pix) if return_parts else loss


def ssim_loss(a, b, data_range=2.0, crop_border=0, luma=False, reduction='mean'):
    """``1 - SSIM`` -> ``image_loss`` with the structural term alone"""
    return image_loss(a, b, ssim_weight=1.0, pixel_weight=0.0, data_range=data_range, crop_border=crop_border, luma=luma,
                      reduction=reduction)


def l1_loss(a, b, crop_border=0, luma=False, reduction='mean'):
    """``mean |a - b|`` per image -> ``image_loss`` with the L1 pixel term alone"""
    return image_loss(a, b, pixel='l1', crop_border=crop_border, luma=luma, reduction=reduction)


def charbonnier_loss(a, b, eps=1e-3, crop_border=0, luma=False, reduction='mean'):
    """``mean sqrt((a - b)^2 + eps^2)`` per image -> ``image_loss`` with the Charbonnier pixel term alone"""
    return image_loss(a, b, pixel='charbonnier', eps=eps, crop_border=crop_border, luma=luma, reduction=reduction)


class _MsSsimLoss(torch.autograd.Function):
    """-> 1 - ms_ssim [N]; ``cfg`` = (N, C, H, W, crop, luma, data_range, weights)"""

    @staticmethod
    def forward(ctx, a, b, cfg):
        a, b = a.detach().contiguous(), b.detach().contiguous()
        ms, terms, pyr_a, pyr_b = ms_ssim_forward(a, b, cfg)
        ctx.save_for_backward(a, b, pyr_a, pyr_b, terms)      # the inputs, their pooled levels and the terms table: nothing else
        ctx.cfg = cfg
        return 1.0 - ms

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        a, b, pyr_a, pyr_b, terms = ctx.saved_tensors
        n, c, h, w, crop, luma, data_range, wts = ctx.cfg
        da, db = _wanted_grads(ctx, a.shape, a.device)
        if da is not None or db is not None:
            lib = L.lib()
            g = g.to(torch.float32).contiguous()
            ws = L.check_count(lib.sisr_ms_ssim_ws_floats(n, c, h, w, crop, luma, len(wts), 2), 'sisr_ms_ssim_ws_floats')
            work = torch.empty(ws, dtype=torch.float32, device=a.device)
            L.check(lib.sisr_ms_ssim_bwd(a.data_ptr(), b.data_ptr(), pyr_a.data_ptr(), pyr_b.data_ptr(), terms.data_ptr(),
                                         g.data_ptr(), n, c, h, w, crop, luma, data_range, len(wts), weights5(wts), work.data_ptr(),
                                         _ptr(da), _ptr(db), _stream()), 'sisr_ms_ssim_bwd')
        return da, db, None


def ms_ssim_loss(a, b, data_range=2.0, crop_border=0, luma=False, weights=MS_SSIM_WEIGHTS, reduction='mean'):
    """``1 - MS-SSIM[n]`` per image of two fp32 [N, C, H, W] batches, C 1 or 3, with the multi-scale SSIM of ``metrics.ms_ssim``
    (M = ``len(weights)`` scales on the crop / luma view; the view needs ``11 << (M - 1)`` pixels a side, so two or three scales fit
    a 96 x 96 patch).  -> 0-dim fp32 device tensor (the mean over the batch), or [N] with ``reduction='none'``.  Differentiable
    with respect to ``a``, ``b`` or both (only what requires a gradient is computed), once; pixels of the cropped border get exact
    zeros, and so does every pixel of an (image, plane) whose score is 0 because a scale's term is not positive.  M + 1 launches
    forward, M backward; saved: the inputs, their pooled levels and the terms table.  Non-contiguous inputs are made contiguous
    first; a bf16 caller casts."""
    what = 'ms_ssim_loss'
    _validate_pair(a, b, what)
    crop, wts = check_ms_ssim(a, b, data_range, crop_border, weights, what=what)
    _check_reduction(reduction, what)
    require_gpu_tensor(a, 'ms_ssim_loss input a')
    require_gpu_tensor(b, 'ms_ssim_loss input b')
    n, c, h, w = a.shape
    loss = _MsSsimLoss.apply(a, b, (n, c, h, w, crop, int(bool(luma)), float(data_range), wts))
    return loss.mean() if reduction == 'mean' else loss


FREQ_KINDS = {'l1': L.FREQ_L1, 'charbonnier': L.FREQ_CHARBONNIER, 'focal': L.FREQ_FOCAL}


class _FreqLoss(torch.autograd.Function):
    """-> loss [N]; ``cfg`` = (N, C, H, W, crop, luma, kind, eps, alpha)"""

    @staticmethod
    def forward(ctx, a, b, cfg):
        a, b = a.detach().contiguous(), b.detach().contiguous()
        n, c, h, w, crop, luma, kind, eps, alpha = cfg
        lib, dev = L.lib(), a.device
        shape = (n, c, h, w, crop, luma)

        def buf(which):
            return torch.empty(L.check_count(lib.sisr_freq_loss_ws_floats(*shape, which), 'sisr_freq_loss_ws_floats'),
                               dtype=torch.float32, device=dev)
        need = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        work, loss = buf(0), torch.empty(n, dtype=torch.float32, device=dev)
        spec = buf(1) if need else None                              # the spectrum D: written only when a gradient will be needed
        pmax = buf(2) if kind == L.FREQ_FOCAL else None
        L.check(lib.sisr_freq_loss_fwd(a.data_ptr(), b.data_ptr(), *shape, kind, eps, alpha, work.data_ptr(),
                                       _ptr(spec), _ptr(pmax), loss.data_ptr(), _stream()), 'sisr_freq_loss_fwd')
        if need:
            ctx.save_for_backward(spec, pmax)  # D and the plane maxima: the inputs are NOT kept
        ctx.cfg, ctx.dims = cfg, (a.shape, dev)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        spec, pmax = ctx.saved_tensors
        n, c, h, w, crop, luma, kind, eps, alpha = ctx.cfg
        shape, dev = ctx.dims
        da, db = _wanted_grads(ctx, shape, dev)
        if da is not None or db is not None:
            lib = L.lib()
            g = g.to(torch.float32).contiguous()
            ws = L.check_count(lib.sisr_freq_loss_ws_floats(n, c, h, w, crop, luma, 3), 'sisr_freq_loss_ws_floats')
            work = torch.empty(ws, dtype=torch.float32, device=dev)
            L.check(lib.sisr_freq_loss_bwd(spec.data_ptr(), _ptr(pmax), g.data_ptr(), n, c, h, w, crop,
                                           luma, kind, eps, alpha, work.data_ptr(), _ptr(da), _ptr(db), _stream()),
                    'sisr_freq_loss_bwd')
        return da, db, None


def frequency_loss(a, b, kind='l1', eps=1e-3, alpha=1.0, crop_border=0, luma=False, reduction='mean'):
    """A frequency-domain loss per image of two fp32 [N, C, H, W] batches, C 1 or 3, on the view of ``metrics`` (``crop_border``
    pixels stripped from every side, then the BT.601 plane with ``luma``: [N, C', H', W']), with ``D`` the unnormalised 2-D DFT of
    ``view(a) - view(b)`` (one transform serves both images):

    ``kind='l1'``: the mean of ``|Re D|`` and ``|Im D|`` over the half spectrum ``torch.fft.rfft2`` returns (BasicSR's ``FFTLoss``:
    ``kw < W' // 2 + 1``, no Hermitian doubling; a component that is exactly 0 has gradient 0).  ``kind='charbonnier'``: the same
    with ``sqrt(z^2 + eps^2)`` per component.  ``kind='focal'``: the focal frequency loss (Jiang et al., ICCV 2021) with
    ``patch_factor=1`` and no ``log_matrix`` / ``ave_spectrum`` / ``batch_matrix``: the mean over the FULL ``norm='ortho'`` spectrum of
    ``w * |D|^2 / (H' W')`` with ``w = |D|^alpha / max |D|^alpha`` per (image, plane), ``w`` a constant for the gradient; an (image,
    plane) with ``a == b`` has loss 0 and an all-zero gradient.

    -> 0-dim fp32 device tensor (the mean over the batch), or [N] with ``reduction='none'``.  Differentiable with respect to ``a``,
    ``b`` or both (only what requires a gradient is computed; pixels of the cropped border get exact zeros; ``db`` is ``-da`` bit
    for bit), once.  View sides 1 .. 256 (a direct separable DFT, csrc/freq_loss.hip: no power-of-two rule).  Three launches forward,
    two backward; the backward does not read the inputs: saved are ``D`` (``N C' H' (W' // 2 + 1) 2`` floats, about one input's
    size) and the plane maxima, and nothing at all when no gradient is required.  Non-contiguous inputs are made contiguous first; a
    bf16 caller casts."""
    what = 'frequency_loss'
    _validate_pair(a, b, what)
    crop = check_view(a, b, 1.0, crop_border, least=1, what=what)
    n, c, h, w = a.shape
    if kind not in FREQ_KINDS:
        raise ValueError('%s: kind is one of %s, got %r' % (what, sorted(FREQ_KINDS), kind))
    _check_reduction(reduction, what)
    if not float(eps) >= 0.0:
        raise ValueError('%s: eps must not be negative, got %r' % (what, eps))
    if not 0.0 < float(alpha) <= 4.0:
        raise ValueError('%s: alpha must lie in (0, 4], got %r' % (what, alpha))
    if max(h, w) - 2 * crop > L.FREQ_MAX_SIDE:
        raise ValueError('%s: %d x %d pixels remain after cropping; the kernels take view sides up to %d'
                         % (what, h - 2 * crop, w - 2 * crop, L.FREQ_MAX_SIDE))
    require_gpu_tensor(a, 'frequency_loss input a')
    require_gpu_tensor(b, 'frequency_loss input b')
    loss = _FreqLoss.apply(a, b, (n, c, h, w, crop, int(bool(luma)), FREQ_KINDS[kind], float(eps), float(alpha)))
    return loss.mean() if reduction == 'mean' else loss


def fft_l1_loss(a, b, crop_border=0, luma=False, reduction='mean'):
    """``mean |rfft2(a) - rfft2(b)|`` over real and imaginary parts per image -> ``frequency_loss`` with ``kind='l1'``"""
    return frequency_loss(a, b, kind='l1', crop_border=crop_border, luma=luma, reduction=reduction)


def focal_frequency_loss(a, b, alpha=1.0, crop_border=0, luma=False, reduction='mean'):
    """the focal frequency loss per image -> ``frequency_loss`` with ``kind='focal'``"""
    return frequency_loss(a, b, kind='focal', alpha=alpha, crop_border=crop_border, luma=luma, reduction=reduction)


def _check_artifact(sr, gt, ema, ksize, what):
    """the argument errors, whatever the tensors live on -> (N, C, H, W)"""
    _validate_pair(sr, gt, what)
    _validate_pair(sr, ema, what)
    if sr.dim() != 4 or sr.shape[1] not in (1, 3):
        raise ValueError('%s: [N, C, H, W] batches with C 1 or 3 are expected, got shape %s' % (what, tuple(sr.shape)))
    if not isinstance(ksize, int) or isinstance(ksize, bool) or ksize < 3 or ksize > L.ARTIFACT_MAX_K or ksize % 2 == 0:
        raise ValueError('%s: ksize is an odd integer in 3 .. %d, got %r' % (what, L.ARTIFACT_MAX_K, ksize))
    h, w = sr.shape[-2:]
    if min(h, w) <= ksize // 2:
        raise ValueError('%s: the mirrored border of a %d x %d window needs sides longer than %d, got %d x %d'
                         % (what, ksize, ksize, ksize // 2, h, w))
    if sr.numel() > 2 ** 31 - 1:
        raise ValueError('%s: at most 2^31 - 1 elements per batch, got %d' % (what, sr.numel()))
    return tuple(sr.shape)


def _require_gpu_artifact(sr, gt, ema, what):
    for t, name in ((sr, 'sr'), (gt, 'gt'), (ema, 'ema')):
        require_gpu_tensor(t, '%s input %s' % (what, name))


def _artifact_forward(sr, gt, ema, shape, ksize, weight, with_loss):
    """-> (map [N, 1, H, W], loss [N] or None) of contiguous detached inputs"""
    n, c, h, w = shape
    lib, dev = L.lib(), sr.device
    work = torch.empty(L.check_count(lib.sisr_artifact_ws_floats(n, h, w), 'sisr_artifact_ws_floats'), dtype=torch.float32, device=dev)
    amap = torch.empty((n, 1, h, w), dtype=torch.float32, device=dev)
    loss = torch.empty(n, dtype=torch.float32, device=dev) if with_loss else None
    L.check(lib.sisr_artifact_fwd(sr.data_ptr(), gt.data_ptr(), ema.data_ptr(), n, c, h, w, ksize, weight, work.data_ptr(),
                                  amap.data_ptr(), _ptr(loss), _stream()), 'sisr_artifact_fwd')
    return amap, loss


class _ArtifactLoss(torch.autograd.Function):
    """-> (loss[N], map[N, 1, H, W]); ``cfg`` = (N, C, H, W, ksize, weight)"""

    @staticmethod
    def forward(ctx, sr, gt, ema, cfg):
        sr, gt, ema = sr.detach().contiguous(), gt.detach().contiguous(), ema.detach().contiguous()
        amap, loss = _artifact_forward(sr, gt, ema, cfg[:4], cfg[4], cfg[5], True)
        ctx.save_for_backward(sr, gt, amap)    # the two inputs and the one-channel map: ema is not kept
        ctx.cfg = cfg
        ctx.mark_non_differentiable(amap)
        return loss, amap

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _g_map):
        sr, gt, amap = ctx.saved_tensors
        n, c, h, w, _, weight = ctx.cfg
        dsr, dgt = _wanted_grads(ctx, sr.shape, sr.device)
        if dsr is not None or dgt is not None:
            g = g.to(torch.float32).contiguous()
            L.check(L.lib().sisr_artifact_bwd(sr.data_ptr(), gt.data_ptr(), amap.data_ptr(), g.data_ptr(), n, c, h, w, weight,
                                              _ptr(dsr), _ptr(dgt), _stream()), 'sisr_artifact_bwd')
        return dsr, dgt, None, None


def artifact_map(gt, sr, ema, ksize=7):
    """The refined artifact map of the LDL loss (BasicSR's ``get_refined_artifact_map(img_gt, img_output, img_ema, ksize)``) of three
    fp32 [N, C, H, W] device batches, C 1 or 3 -> a detached fp32 [N, 1, H, W] tensor; no graph is recorded.  With
    ``r_sr = sum_c |gt - sr|`` and ``r_ema = sum_c |gt - ema|``: the unbiased variance of ``r_sr`` over the ``ksize`` x ``ksize``
    window of each pixel (mirrored border, torch's ``reflect``) times ``Var(r_sr[n])^(1/5)`` over the whole sample, and exactly 0
    where ``r_sr < r_ema`` (strict: a tie keeps the weight, so ``ema is sr`` masks nothing).  ``ksize`` odd, 3 .. 11; H and W
    longer than ``ksize // 2``."""
    shape = _check_artifact(sr, gt, ema, ksize, 'artifact_map')
    _require_gpu_artifact(sr, gt, ema, 'artifact_map')
    with torch.no_grad():
        return _artifact_forward(sr.detach().contiguous(), gt.detach().contiguous(), ema.detach().contiguous(), shape, ksize, 1.0,
                                 False)[0]


def artifact_loss(sr, gt, ema, ksize=7, weight=1.0, reduction='mean', return_map=False):
    """The artifact-aware (LDL) loss of Liang et al. (CVPR 2022) per image of fp32 [N, C, H, W] device batches, C 1 or 3:
    ``weight * mean_{c,y,x}(m * |sr - gt|)`` with ``m = artifact_map(gt, sr, ema, ksize)`` -- BasicSR's
    ``L1Loss(m * sr, m * gt)``, as ``m >= 0``.  ``ema`` is the output of the EMA generator on the same input.
    -> 0-dim fp32 device tensor (the mean over the batch), or [N] with ``reduction='none'``; with ``return_map`` also the detached
    map.

    THE MAP IS A CONSTANT OF THE LOSS (detached): ``dL/dsr = g[n] * weight * m * sign(sr - gt) / (C H W)``, ``dL/dgt = -dL/dsr``
    bit for bit, ``sign(0) = 0``, and ``ema`` gets no gradient.  A gradient through the map (through the two variances) is left
    out on purpose: the map is a weighting, not a term to be minimised.  Differentiable with respect to ``sr``, ``gt`` or both
    (only what requires a gradient is computed), once.  Three launches forward, one backward; saved: ``sr``, ``gt`` and the map.
    Non-contiguous inputs are made contiguous first; a bf16 caller casts."""
    what = 'artifact_loss'
    shape = _check_artifact(sr, gt, ema, ksize, what)
    _check_reduction(reduction, what)
    weight = float(weight)
    if not np.isfinite(weight):
        raise ValueError('%s: weight must be finite, got %r' % (what, weight))
    _require_gpu_artifact(sr, gt, ema, what)
    loss, amap = _ArtifactLoss.apply(sr, gt, ema, shape + (ksize, weight))
    if reduction == 'mean':
        loss = loss.mean()
    return (loss, amap) if return_map else loss


PERCEP_CRITERIA = {'l1': L.PERCEP_L1, 'l2': L.PERCEP_L2, 'fro': L.PERCEP_FRO}


def _check_taps(feat, shapes, what):
    """the argument errors of a (B, total) feature tensor and its tap shapes -> ((C, H, W), ...) of ints"""
    if feat.dim() != 2:
        raise ValueError('%s: a (B, total) feature tensor is expected, got shape %s' % (what, tuple(feat.shape)))
    try:
        taps = tuple(tuple(int(v) for v in s) for s in shapes)
    except (TypeError, ValueError):
        raise ValueError('%s: shapes is a sequence of (C, H, W), got %r' % (what, shapes)) from None
    if not 1 <= len(taps) <= L.PERCEP_MAX_TAPS:
        raise ValueError('%s: 1 .. %d taps are expected, got %d' % (what, L.PERCEP_MAX_TAPS, len(taps)))
    if any(len(s) != 3 or min(s) < 1 for s in taps):
        raise ValueError('%s: every shape is (C, H, W) with positive sizes, got %r' % (what, taps))
    if any(s[0] * s[1] * s[2] > 2 ** 31 - 1 for s in taps):
        raise ValueError('%s: at most 2^31 - 1 elements per tap and sample, got %r' % (what, taps))
    total = sum(c * h * w for c, h, w in taps)
    if total != feat.shape[1]:
        raise ValueError('%s: the shapes %r hold %d elements per sample, the tensor has %d' % (what, taps, total, feat.shape[1]))
    return taps


def _tap_array(taps):
    return (L._i32 * (3 * len(taps)))(*[v for s in taps for v in s])


def _percep_work(lib, b, taps, with_feature, with_style, dev):
    size = L.check_count(lib.sisr_percep_ws_bytes(b, len(taps), _tap_array(taps), int(with_feature), int(with_style)),
                         'sisr_percep_ws_bytes')
    return torch.empty(max(size, 16) // 4, dtype=torch.float32, device=dev)


def _gram_forward(feat, taps):
    """-> the taps' (B, C, C) Gram matrices of a contiguous detached (B, total) tensor: views of one buffer"""
    lib, dev, b = L.lib(), feat.device, feat.shape[0]
    work = _percep_work(lib, b, taps, False, True, dev)
    out = torch.empty(sum(b * c * c for c, _, _ in taps), dtype=torch.float32, device=dev)
    L.check(lib.sisr_percep_gram(feat.data_ptr(), b, feat.shape[1], len(taps), _tap_array(taps), work.data_ptr(), out.data_ptr(),
                                 _stream()), 'sisr_percep_gram')
    grams, off = [], 0
    for c, _, _ in taps:
        grams.append(out[off:off + b * c * c].view(b, c, c))
        off += b * c * c
    return tuple(grams)


def gram_matrix(feat, shapes):
    """The Gram matrices ``F F^T / (C H W)`` (BasicSR's ``_gram_mat``) of every tap of a fp32 (B, total) device feature tensor in the
    layout of ``MaskedVGG.forward``; ``shapes``: the taps' ``(C, H, W)``, as ``model_content_extractor.tap_shapes`` returns them.
    -> a tuple of detached (B, C, C) tensors, bit-symmetric and the same bits ``perceptual_loss`` forms internally; no graph is
    recorded.  Two launches for all taps and samples."""
    what = 'gram_matrix'
    _check_tensor(feat, what)
    taps = _check_taps(feat, shapes, what)
    require_gpu_tensor(feat, 'gram_matrix input')
    with torch.no_grad():
        return _gram_forward(feat.detach().contiguous(), taps)


class _Perceptual(torch.autograd.Function):
    """-> (perceptual or None, style or None, terms_p or None, terms_s or None); ``cfg`` = (taps, layer_weights, pw, sw, crit)"""

    @staticmethod
    def forward(ctx, fa, fb, cfg):
        fa, fb = fa.detach().contiguous(), fb.detach().contiguous()
        taps, lw, pw, sw, crit = cfg
        lib, dev, b = L.lib(), fa.device, fa.shape[0]
        need = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        work = _percep_work(lib, b, taps, pw != 0.0, sw != 0.0, dev)
        percep, terms_p = (_scalar(dev), torch.empty(len(taps), dtype=torch.float32, device=dev)) if pw != 0.0 else (None, None)
        style, terms_s = (_scalar(dev), torch.empty(len(taps), dtype=torch.float32, device=dev)) if sw != 0.0 else (None, None)
        # D = dS / dG_a, written only when a gradient will be needed
        dmat = torch.empty(sum(b * c * c for c, _, _ in taps), dtype=torch.float32, device=dev) if need and sw != 0.0 else None
        L.check(lib.sisr_percep_fwd(fa.data_ptr(), fb.data_ptr(), b, fa.shape[1], len(taps), _tap_array(taps),
                                    (L._f32 * len(taps))(*lw), pw, sw, crit, work.data_ptr(), _ptr(terms_p), _ptr(terms_s),
                                    _ptr(percep), _ptr(style), _ptr(dmat), _stream()), 'sisr_percep_fwd')
        if need:
            ctx.save_for_backward(fa, fb, dmat, terms_p, terms_s)      # the inputs, D and the per-tap terms (the 'fro' norms)
        ctx.cfg = cfg
        ctx.mark_non_differentiable(*[t for t in (terms_p, terms_s) if t is not None])
        return percep, style, terms_p, terms_s

    @staticmethod
    @once_differentiable
    def backward(ctx, g_p, g_s, _g_tp, _g_ts):
        fa, fb, dmat, terms_p, terms_s = ctx.saved_tensors
        taps, lw, pw, sw, crit = ctx.cfg
        dfa, dfb = _wanted_grads(ctx, fa.shape, fa.device)
        if dfa is not None or dfb is not None:
            g_p = None if pw == 0.0 else g_p.to(torch.float32).contiguous()
            g_s = None if sw == 0.0 else g_s.to(torch.float32).contiguous()
            L.check(L.lib().sisr_percep_bwd(fa.data_ptr(), fb.data_ptr(), _ptr(dmat), _ptr(terms_p), _ptr(terms_s), _ptr(g_p),
                                            _ptr(g_s), fa.shape[0], fa.shape[1], len(taps), _tap_array(taps),
                                            (L._f32 * len(taps))(*lw), pw, sw, crit, _ptr(dfa), _ptr(dfb), _stream()),
                    'sisr_percep_bwd')
        return dfa, dfb, None


def perceptual_loss(fa, fb, shapes, layer_weights=None, perceptual_weight=1.0, style_weight=0.0, criterion='l1', return_terms=False):
    """BasicSR's ``PerceptualLoss`` on two fp32 (B, total) device feature tensors in the layout of ``MaskedVGG.forward`` (tap ``l`` is
    columns ``[off_l, off_l + C_l H_l W_l)`` of every row in NCHW order); ``shapes``: the taps' ``(C, H, W)``, as
    ``model_content_extractor.tap_shapes`` returns them, at most 8.  Per tap, with ``crit`` the mean of ``|d|`` ('l1'), the mean of
    ``d^2`` ('l2') or ``sqrt(sum d^2)`` over the whole batch tensor of the tap ('fro'):

    ``perceptual = perceptual_weight * sum_l w_l * crit(fa_l, fb_l)`` and ``style = style_weight * sum_l w_l * crit(G(fa_l), G(fb_l))``
    with ``G = F F^T / (C H W)`` per sample (``gram_matrix``) and ``w = layer_weights`` (ones by default).

    -> ``(perceptual, style)``, 0-dim fp32 device tensors; a term whose weight is 0 is ``None`` and none of its launches happen.  With
    ``return_terms`` also the two detached ``[n_taps]`` tables of the unweighted per-tap terms.  Differentiable with respect to
    ``fa``, ``fb`` or both (only what requires a gradient is computed), once; ``sign(0) = 0``, a zero Frobenius norm gives an
    all-zero gradient, a NaN in gives NaN terms.  Four launches forward with both terms, one backward; saved: the inputs, ``D`` (the
    style term's derivative with respect to the Gram matrices, ``B C^2`` floats per tap) and the per-tap terms -- neither ``a - b``
    nor the Gram matrices.  Non-contiguous inputs are made contiguous first; a bf16 caller casts."""
    what = 'perceptual_loss'
    _validate_pair(fa, fb, what)
    taps = _check_taps(fa, shapes, what)
    if layer_weights is None:
        layer_weights = (1.0,) * len(taps)
    lw = tuple(float(v) for v in layer_weights)
    if len(lw) != len(taps):
        raise ValueError('%s: one layer weight per tap is expected, got %d for %d taps' % (what, len(lw), len(taps)))
    pw, sw = float(perceptual_weight), float(style_weight)
    if not all(np.isfinite(v) for v in lw + (pw, sw)):
        raise ValueError('%s: the weights must be finite, got %r, %r, %r' % (what, lw, pw, sw))
    if criterion not in PERCEP_CRITERIA:
        raise ValueError('%s: criterion is one of %s, got %r' % (what, sorted(PERCEP_CRITERIA), criterion))
    require_gpu_tensor(fa, 'perceptual_loss input fa')
    require_gpu_tensor(fb, 'perceptual_loss input fb')
    if pw == 0.0 and sw == 0.0:
        out = (None, None, None, None)
    else:
        out = _Perceptual.apply(fa, fb, (taps, lw, pw, sw, PERCEP_CRITERIA[criterion]))
    return out if return_terms else out[:2]


class PerceptualLoss(torch.nn.Module):
    """BasicSR's ``PerceptualLoss`` around a content extractor of ``model_content_extractor`` (``MaskedVGG``, ``vgg_4conv_1maxPool``
    or ``identity()``): ``forward(x, gt)`` -> ``(percep, style)`` of ``perceptual_loss`` on the extractor's features, the tap shapes
    taken from ``tap_shapes``.  ``gt``'s features are computed under ``no_grad``.  ``range_norm`` maps [-1, 1] images to [0, 1] and
    ``input_norm`` applies the ImageNet mean / std, as BasicSR's ``VGGFeatureExtractor`` does (a per-channel affine on the
    3-channel image: torch ops, not the hot path).  The Real-ESRGAN setting: ``MaskedVGG(0b11111)``, ``layer_weights=(0.1, 0.1, 1,
    1, 1)``, ``criterion='l1'``."""

    def __init__(self, extractor, layer_weights=None, perceptual_weight=1.0, style_weight=0.0, criterion='l1', input_norm=False,
                 range_norm=False):
        super().__init__()
        if criterion not in PERCEP_CRITERIA:
            raise ValueError('PerceptualLoss: criterion is one of %s, got %r' % (sorted(PERCEP_CRITERIA), criterion))
        self.extractor = extractor
        self.layer_weights = None if layer_weights is None else tuple(float(v) for v in layer_weights)
        self.perceptual_weight, self.style_weight, self.criterion = float(perceptual_weight), float(style_weight), criterion
        self.input_norm, self.range_norm = bool(input_norm), bool(range_norm)
        self.register_buffer('mean', torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1), persistent=False)
        self.register_buffer('std', torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1), persistent=False)

    def _features(self, x):
        if self.range_norm:
            x = (x + 1) / 2
        if self.input_norm:
            x = (x - self.mean.to(x.device)) / self.std.to(x.device)
        return self.extractor(x).reshape(x.shape[0], -1)

    def forward(self, x, gt):
        from .model_content_extractor import tap_shapes
        shapes = tap_shapes(self.extractor, x.shape[2], x.shape[3])
        fx = self._features(x)
        with torch.no_grad():
            fg = self._features(gt.detach())
        return perceptual_loss(fx, fg, shapes, self.layer_weights, self.perceptual_weight, self.style_weight, self.criterion)


def _cx_check_taps(feat, shapes, what):
    taps = _check_taps(feat, shapes, what)
    if any(h * w > L.CX_MAX_POINTS for _, h, w in taps):
        raise ValueError('%s: at most %d points (H * W) per tap, got %r: take a deeper tap or pool the features first'
                         % (what, L.CX_MAX_POINTS, taps))
    return taps


def _cx_buffer(lib, b, taps, which, dev):
    size = L.check_count(lib.sisr_cx_ws_bytes(b, len(taps), _tap_array(taps), which), 'sisr_cx_ws_bytes')
    return torch.empty(max(size, 16) // 4, dtype=torch.float32, device=dev)


def _cx_table_views(tab, b, taps):
    """-> per tap a dict of views of the tables buffer: mu [C]; na, nb, m, Z, c (fp32) and jstar, istar (int32), each (B, P)"""
    n_mu, n_pt = sum(c for c, _, _ in taps), b * sum(h * w for _, h, w in taps)
    names = ('na', 'nb', 'm', 'Z', 'c', 'jstar', 'istar')
    out, mu, pt = [], 0, 0
    for c, h, w in taps:
        p = h * w
        d = {'mu': tab[mu:mu + c]}
        for k, name in enumerate(names):
            v = tab[n_mu + k * n_pt + pt:n_mu + k * n_pt + pt + b * p].view(b, p)
            d[name] = v.view(torch.int32) if name in ('jstar', 'istar') else v
        out.append(d)
        mu, pt = mu + c, pt + b * p
    return tuple(out)


def _cx_forward(fa, fb, taps, lw, h, weight):
    """the forward on contiguous detached tensors -> (loss, terms [n_taps], cx [n_taps, B], tables buffer); the P^2 workspace is
    released on return"""
    lib, dev, b = L.lib(), fa.device, fa.shape[0]
    tab = _cx_buffer(lib, b, taps, L.CX_WS_TABLES, dev)
    work = _cx_buffer(lib, b, taps, L.CX_WS_FWD, dev)
    loss, terms = _scalar(dev), torch.empty(len(taps), dtype=torch.float32, device=dev)
    cx = torch.empty((len(taps), b), dtype=torch.float32, device=dev)
    L.check(lib.sisr_cx_fwd(fa.data_ptr(), fb.data_ptr(), b, fa.shape[1], len(taps), _tap_array(taps), (L._f32 * len(taps))(*lw), h,
                            weight, tab.data_ptr(), work.data_ptr(), terms.data_ptr(), cx.data_ptr(), loss.data_ptr(), _stream()),
            'sisr_cx_fwd')
    return loss, terms, cx, tab


class _Contextual(torch.autograd.Function):
    """-> (loss, terms, cx); ``cfg`` = (taps, layer_weights, band_width, weight)"""

    @staticmethod
    def forward(ctx, fa, fb, cfg):
        fa, fb = fa.detach().contiguous(), fb.detach().contiguous()
        taps, lw, h, weight = cfg
        loss, terms, cx, tab = _cx_forward(fa, fb, taps, lw, h, weight)
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(fa, fb, tab, cx)                 # the inputs, the O(B P) tables with mu, CX[n]: nothing of size P^2
        ctx.cfg = cfg
        ctx.mark_non_differentiable(terms, cx)
        return loss, terms, cx

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _g_terms, _g_cx):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        fa, fb, tab, cx = ctx.saved_tensors
        taps, lw, h, weight = ctx.cfg
        lib, dev, b = L.lib(), fa.device, fa.shape[0]
        g = g.to(torch.float32).contiguous()
        work = _cx_buffer(lib, b, taps, L.CX_WS_BWD, dev)
        dfa = torch.empty_like(fa)
        L.check(lib.sisr_cx_bwd(fa.data_ptr(), fb.data_ptr(), tab.data_ptr(), cx.data_ptr(), g.data_ptr(), b, fa.shape[1], len(taps),
                                _tap_array(taps), (L._f32 * len(taps))(*lw), h, weight, work.data_ptr(), dfa.data_ptr(), _stream()),
                'sisr_cx_bwd')
        return dfa, None, None


def _cx_args(fa, fb, shapes, layer_weights, band_width, weight, what):
    """the argument errors of ``contextual_loss`` -> (taps, lw, h, weight)"""
    _validate_pair(fa, fb, what)
    taps = _cx_check_taps(fa, shapes, what)
    if layer_weights is None:
        layer_weights = (1.0,) * len(taps)
    lw = tuple(float(v) for v in layer_weights)
    if len(lw) != len(taps):
        raise ValueError('%s: one layer weight per tap is expected, got %d for %d taps' % (what, len(lw), len(taps)))
    h, weight = float(band_width), float(weight)
    if not all(np.isfinite(v) for v in lw + (weight,)):
        raise ValueError('%s: the weights must be finite, got %r, %r' % (what, lw, weight))
    if not np.finfo(np.float32).tiny <= h <= np.finfo(np.float32).max:      # (a NaN fails both comparisons)
        raise ValueError('%s: band_width is a finite positive fp32 number, got %r' % (what, band_width))
    return taps, lw, h, weight


def contextual_loss(fa, fb, shapes, layer_weights=None, band_width=0.5, weight=1.0, return_terms=False):
    """The contextual loss of Mechrez, Talmi and Zelnik-Manor (ECCV 2018) in its cosine form on two fp32 (B, total) device feature
    tensors in the layout of ``MaskedVGG.forward``; ``shapes``: the taps' ``(C, H, W)`` as ``perceptual_loss`` takes them, at most 8,
    each with ``P = H W <= 2304`` points (conv2_2 at HR 96^2, conv3_4 at HR 192^2; above that take a deeper tap or pool the features).
    ``fa`` is the generator side, ``fb`` the target; the roles are not symmetric.  Per tap and sample, with ``x_i`` / ``y_j`` the
    feature points (columns of the C x P slices), ``mu`` the channel-wise mean of the TARGET over batch and points and ``h =
    band_width``:

    ``S_ij = cos(x_i - mu, y_j - mu)`` (norms clamped at 1e-12), ``d = 1 - S``, ``w_ij = exp((1 - d_ij / (min_j d_ij + 1e-5)) / h)``,
    ``CX_ij = w_ij / sum_j w_ij``, ``CX[n] = mean_j max_i CX_ij``, ``loss = weight * sum_l w_l * mean_n -log(CX[n] + 1e-5)``.

    -> a 0-dim fp32 device tensor; with ``return_terms`` also the detached ``[n_taps]`` per-tap terms and the ``[n_taps, B]`` table of
    ``CX[n]``.  Differentiable with respect to ``fa`` only, once: ``fb`` is a constant of the loss (detached, as ``ema`` is in
    ``artifact_loss``) and gets no gradient.  Ties of the min and of the max take the lowest index.  ``P = 1`` gives ``CX = 1`` and a
    zero gradient; when ``fa`` is close to ``fb`` the loss saturates at ``-log(1 + 1e-5)`` and the gradient underflows to 0 -- the
    definition's behaviour, not an error; a NaN in gives a NaN term.  Six launches forward, four backward, none depending on B; saved
    are the inputs, the O(B P) tables and ``CX[n]`` -- the ``B P^2`` similarity lives in a workspace that is released after each pass
    and is recomputed in the backward.  Non-contiguous inputs are made contiguous first; a bf16 caller casts."""
    what = 'contextual_loss'
    cfg = _cx_args(fa, fb, shapes, layer_weights, band_width, weight, what)
    require_gpu_tensor(fa, 'contextual_loss input fa')
    require_gpu_tensor(fb, 'contextual_loss input fb')
    out = _Contextual.apply(fa, fb, cfg)
    return out if return_terms else out[0]


def contextual_similarity(fa, fb, shapes):
    """The cosine similarities ``S_ij`` of ``contextual_loss`` for every tap of two fp32 (B, total) device feature tensors -> a tuple
    of detached (B, P, P) tensors (row ``i``: a point of ``fa``, column ``j``: a point of ``fb``), the same bits the loss forms
    internally; no graph is recorded.  Three launches for all taps and samples."""
    what = 'contextual_similarity'
    _validate_pair(fa, fb, what)
    taps = _cx_check_taps(fa, shapes, what)
    require_gpu_tensor(fa, 'contextual_similarity input fa')
    require_gpu_tensor(fb, 'contextual_similarity input fb')
    with torch.no_grad():
        fa, fb = fa.detach().contiguous(), fb.detach().contiguous()
        lib, dev, b = L.lib(), fa.device, fa.shape[0]
        tab = _cx_buffer(lib, b, taps, L.CX_WS_TABLES, dev)
        out = _cx_buffer(lib, b, taps, L.CX_WS_SIM, dev)
        L.check(lib.sisr_cx_sim(fa.data_ptr(), fb.data_ptr(), b, fa.shape[1], len(taps), _tap_array(taps), tab.data_ptr(),
                                out.data_ptr(), _stream()), 'sisr_cx_sim')
        sims, off = [], 0
        for _, h, w in taps:
            p = h * w
            sims.append(out[off:off + b * p * p].view(b, p, p))
            off += b * p * p
        return tuple(sims)


def _contextual_tables(fa, fb, shapes, band_width=0.5):
    """The tables the forward leaves for the backward, for the tests -> per tap a dict (``_cx_table_views``)"""
    taps, lw, h, weight = _cx_args(fa, fb, shapes, None, band_width, 1.0, 'contextual tables')
    require_gpu_tensor(fa, 'contextual tables input fa')
    with torch.no_grad():
        tab = _cx_forward(fa.detach().contiguous(), fb.detach().contiguous(), taps, lw, h, weight)[3]
    return _cx_table_views(tab, fa.shape[0], taps)


class ContextualLoss(torch.nn.Module):
    """``contextual_loss`` around a content extractor of ``model_content_extractor``, beside ``PerceptualLoss``: ``forward(x, gt)`` ->
    the loss on the extractor's features, the tap shapes taken from ``tap_shapes``.  ``gt``'s features are computed under ``no_grad``
    and are a constant of the loss.  ``range_norm`` / ``input_norm`` as in ``PerceptualLoss``.  A setting for HR 96^2 patches:
    ``MaskedVGG(0b01100)`` (conv3_4 and conv4_4: 576 and 144 points)."""

    def __init__(self, extractor, layer_weights=None, band_width=0.5, weight=1.0, input_norm=False, range_norm=False):
        super().__init__()
        h = float(band_width)
        if not np.finfo(np.float32).tiny <= h <= np.finfo(np.float32).max:
            raise ValueError('ContextualLoss: band_width is a finite positive fp32 number, got %r' % (band_width,))
        self.extractor = extractor
        self.layer_weights = None if layer_weights is None else tuple(float(v) for v in layer_weights)
        self.band_width, self.weight = h, float(weight)
        self.input_norm, self.range_norm = bool(input_norm), bool(range_norm)
        self.register_buffer('mean', torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1), persistent=False)
        self.register_buffer('std', torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1), persistent=False)

    _features = PerceptualLoss._features

    def forward(self, x, gt):
        from .model_content_extractor import tap_shapes
        shapes = tap_shapes(self.extractor, x.shape[2], x.shape[3])
        fx = self._features(x)
        with torch.no_grad():
            fg = self._features(gt.detach())
        return contextual_loss(fx, fg, shapes, self.layer_weights, self.band_width, self.weight)


class _BCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p, t_vec, t_scalar, weight):
        p = p.detach().contiguous()
        t_vec = None if t_vec is None else t_vec.detach().contiguous()
        loss, mean_p = _scalar(p.device), _scalar(p.device)
        L.check(L.lib().sisr_bce_fwd(p.data_ptr(), _ptr(t_vec), t_scalar, p.numel(), weight,
                                     loss.data_ptr(), mean_p.data_ptr(), _stream()), 'sisr_bce_fwd')
        ctx.save_for_backward(p, t_vec)
        ctx.t_scalar, ctx.weight = t_scalar, weight
        ctx.mark_non_differentiable(mean_p)
        return loss, mean_p

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _g_mean):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        p, t_vec = ctx.saved_tensors
        g = g.to(torch.float32).contiguous()
        dp = torch.empty_like(p)
        L.check(L.lib().sisr_bce_bwd(p.data_ptr(), _ptr(t_vec), ctx.t_scalar, p.numel(),
                                     ctx.weight, g.data_ptr(), dp.data_ptr(), _stream()), 'sisr_bce_bwd')
        return dp, None, None, None


def bce_loss(p, target, weight=1.0, return_mean=False):
    """``weight * F.binary_cross_entropy(p, target)`` (mean reduction, log terms clamped at -100 as torch does) -> 0-dim fp32
    device tensor, or ``(loss, mean(p))`` with ``return_mean``.  ``target``: a Python number (one label for every element, as the
    reference's ``torch.full`` label tensors) or a tensor of ``p``'s shape; no gradient flows to it.  Elements of ``p`` outside
    [0, 1] or NaN give a NaN loss, not a device-side assertion."""
    _check_tensor(p, 'bce_loss input')
    if isinstance(target, torch.Tensor):
        _validate_pair(p, target, 'bce_loss')
        t_vec, t_scalar = target, 0.0
    elif isinstance(target, (int, float)):
        t_vec, t_scalar = None, float(target)
    else:
        raise ValueError('bce_loss: the target is a number or a tensor of the shape of the input, got %s' % type(target))
    require_gpu_tensor(p, 'bce_loss input')
    if t_vec is not None:
        require_gpu_tensor(t_vec, 'bce_loss target')
    loss, mean_p = _BCE.apply(p, t_vec, t_scalar, float(weight))
    return (loss, mean_p) if return_mean else loss


class BCELoss(torch.nn.Module):
    """``torch.nn.BCELoss`` as the reference uses it (config.py:107: no rescaling weight, mean reduction) on ``bce_loss``"""

    def __init__(self, weight=None, size_average=None, reduce=None, reduction='mean'):
        super().__init__()
        if weight is not None or size_average is not None or reduce is not None or reduction != 'mean':
            raise NotImplementedError("fused BCELoss: only weight=None, reduction='mean' are implemented "
                                      '(the reference uses nothing else, config.py:107)')

    def forward(self, input, target):
        return bce_loss(input, target)


# ---- the loss functions of train.py:128-186; the D statistics come back as device tensors (no .item()) ------------------------
def content_loss_g(content_extractor, real, fake, weight=1.0):
    """train.py:183-186 -> weight * mean((extractor(real) - extractor(fake))^2)"""
    return feature_mse(content_extractor(real), content_extractor(fake), weight)


def adversarial_loss_g(net_d, fake, real_label=1.0, weight=1.0):
    """train.py:171-181 -> (D_G_z2, errG), errG already times ``weight`` (train.py:88)"""
    err, d_g_z2 = bce_loss(net_d(fake).view(-1), real_label, weight, return_mean=True)
    return d_g_z2, err


def adversarial_loss_d(net_d, real, curr_fake, old_fakes, ratio=0.01, real_label=0.9, fake_label=0.0, weight=1.0):
    """The D-step loss of train.py:128-168 over ``[curr_fake] + sampled old fakes`` (every batch is its own D forward: its own
    BatchNorm statistics and spectral-norm iteration, as in the reference).  ``old_fakes``: a ``replay.DeviceReplayList`` (sampled
    through its ``sample``) or a plain list (sampled with ``np.random.choice`` exactly as train.py:144-146: the same draw from the
    same generator either way).  -> (D_G_z1, D_x, errD), errD already times ``weight`` (train.py:73)"""
    err, d_x = bce_loss(net_d(real).view(-1), real_label, weight, return_mean=True)
    if hasattr(old_fakes, 'sample'):
        sampled = old_fakes.sample(ratio)
    else:
        idx = np.random.choice(list(range(len(old_fakes))), int(len(old_fakes) * ratio), replace=False)
        sampled = [old_fakes[int(i)] for i in idx]
    d_g_z1 = None
    for fake in [curr_fake] + sampled:
        e, m = bce_loss(net_d(fake).view(-1), fake_label, weight, return_mean=True)
        err = err + e
        d_g_z1 = m if d_g_z1 is None else d_g_z1 + m
    return d_g_z1, d_x, err
