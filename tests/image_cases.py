"""Inputs and the float64 definition shared by test_gpu_metrics.py and test_gpu_image_loss.py (a plain module, not a conftest).

Inputs are structured (a smooth pattern per image and plane, plus noise whose strength grows along x, never constant: a != b
everywhere), so that an indexing mistake moves the result.  The definition is written with torch ops in the dtype of its inputs:

    loss[n] = w_ssim (1 - SSIM[n]) + w_pix mean_{C',H',W'} rho(a - b),   rho = |d| / sqrt(d^2 + eps^2) / d^2

on the crop / luma view, SSIM with the separable 11-tap Gaussian (sigma 1.5) through F.conv2d at the "valid" positions."""
import functools

import torch
import torch.nn.functional as F

WINDOW = 11


@functools.lru_cache(maxsize=None)
def _images(shape, seed=0):
    """(a, b) fp32 CPU tensors in [-1, 1]; never modified"""
    n, c, h, w = shape
    y = torch.linspace(0, 1, h, dtype=torch.float64).view(1, 1, h, 1)
    x = torch.linspace(0, 1, w, dtype=torch.float64).view(1, 1, 1, w)
    i = torch.arange(n, dtype=torch.float64).view(n, 1, 1, 1)
    k = torch.arange(c, dtype=torch.float64).view(1, c, 1, 1)
    base = 0.8 * torch.sin(3 * (i + 1) * x + 2 * (k + 1) * y + i) * (0.3 + 0.7 * y)
    noise = torch.randn(shape, dtype=torch.float64, generator=torch.Generator().manual_seed(1234 + seed))
    a = base.clamp(-1, 1)
    b = (base + noise * (0.02 + 0.25 * x)).clamp(-1, 1)
    return a.float(), b.float()


def _view(t, crop, luma):
    if crop:
        t = t[:, :, crop:t.shape[2] - crop, crop:t.shape[3] - crop]
    if luma and t.shape[1] == 3:
        t = (0.299 * t[:, 0] + 0.587 * t[:, 1] + 0.114 * t[:, 2]).unsqueeze(1)
    return t


def _definition(a, b, ssim_weight=0.0, pixel_weight=1.0, pixel='l1', eps=1e-3, data_range=2.0, crop_border=0, luma=False):
    """the loss as torch ops in the dtype of a and b -> (loss [N], ssim [N] or None, pix [N]); differentiable"""
    a, b = _view(a, crop_border, luma), _view(b, crop_border, luma)
    n, c, h, w = a.shape
    d = a - b
    rho = d.abs() if pixel == 'l1' else torch.sqrt(d * d + eps * eps) if pixel == 'charbonnier' else d * d
    pix = rho.mean(dim=(1, 2, 3))
    loss, ssim = pixel_weight * pix, None
    if min(h, w) >= WINDOW:
        g = torch.exp(-(torch.arange(WINDOW, dtype=torch.float64) - WINDOW // 2) ** 2 / (2 * 1.5 ** 2))
        g = (g / g.sum()).to(a)

        def win(t):
            t = t.reshape(n * c, 1, h, w)
            return F.conv2d(F.conv2d(t, g.view(1, 1, WINDOW, 1)), g.view(1, 1, 1, WINDOW))
        c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
        mu_a, mu_b = win(a), win(b)
        var_a, var_b, cov = win(a * a) - mu_a ** 2, win(b * b) - mu_b ** 2, win(a * b) - mu_a * mu_b
        m = ((2 * mu_a * mu_b + c1) * (2 * cov + c2)) / ((mu_a ** 2 + mu_b ** 2 + c1) * (var_a + var_b + c2))
        assert m.shape[-2:] == (h - 10, w - 10)
        ssim = m.reshape(n, -1).mean(dim=1)
        if ssim_weight != 0.0:
            loss = loss + ssim_weight * (1 - ssim)
    else:
        assert ssim_weight == 0.0
    return loss, ssim, pix
