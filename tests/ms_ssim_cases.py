"""The multi-scale SSIM definition shared by test_ms_ssim_cpu.py and test_gpu_ms_ssim.py (a plain module, not a conftest), written
with torch ops in the dtype of its inputs; inputs and the crop / luma view come from image_cases.py.

    a_0, b_0 = the view planes;   a_{j+1} = F.avg_pool2d(a_j, 2)   (2 x 2 mean, stride 2, no padding: an odd row / column is dropped)
    per window position of level j (separable 11-tap Gaussian, sigma 1.5, through F.conv2d at the "valid" positions):
        cs = (2 s_ab + C2) / (s_a^2 + s_b^2 + C2),   l = (2 mu_a mu_b + C1) / (mu_a^2 + mu_b^2 + C1)
    t_j[n,p] = mean of cs (j < M - 1), mean of l cs (j = M - 1)
    MS[n,p]  = prod_j t_j^{w_j} when every t_j[n,p] > 0, else exactly 0 (with a zero gradient);   ms_ssim[n] = mean_p MS[n,p]

The value cases of the GPU test (shape, weights, crop, luma) live here too, so that the CPU test can state what evaluating the
definition in fp32 instead of fp64 does on exactly those cases."""
import functools

import torch
import torch.nn.functional as F

from image_cases import WINDOW, _images, _view

MS_SSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)

# (shape, weights, crop, luma): each the smallest shape at which one thing can go wrong
VALUE_CASES = [
    ((1, 1, 11, 11), (1.0,), 0, False),                       # (a) one window position, no pyramid
    ((2, 3, 22, 23), MS_SSIM_WEIGHTS[:2], 0, False),          # (b) level 1 is exactly 11 x 11; the odd column is dropped
    ((2, 3, 45, 70), MS_SSIM_WEIGHTS[:2], 0, False),          # (c) ragged tiles, pooled seams at the 16th / 32nd pixel, odd height
    ((2, 3, 45, 70), MS_SSIM_WEIGHTS[:2], 1, False),          # (c) ... the crop shifts the cell parity
    ((2, 3, 47, 71), MS_SSIM_WEIGHTS[:2], 2, True),           # (d) luma with crop and odd sizes
    ((1, 3, 96, 192), MS_SSIM_WEIGHTS[:3], 0, False),         # (e) 6 x 6 tiles
    ((1, 3, 96, 192), MS_SSIM_WEIGHTS[:4], 4, True),          # (e) 6 x 6 tiles, three pooled levels
    ((1, 1, 176, 176), MS_SSIM_WEIGHTS, 0, False),            # (f) the last level is one window position
    ((1, 3, 177, 210), MS_SSIM_WEIGHTS, 0, False),            # (g) five levels, odd sizes at levels 0 and 1
    ((1, 3, 185, 218), MS_SSIM_WEIGHTS, 4, True),             # (g) five levels, crop and luma, odd sizes
]


def _ms_definition(a, b, weights=MS_SSIM_WEIGHTS, data_range=2.0, crop_border=0, luma=False):
    """multi-scale SSIM as torch ops in the dtype of a and b -> (ms_ssim [N], terms [M, N, C']); differentiable"""
    a, b = _view(a, crop_border, luma), _view(b, crop_border, luma)
    g = torch.exp(-(torch.arange(WINDOW, dtype=torch.float64) - WINDOW // 2) ** 2 / (2 * 1.5 ** 2))
    g = (g / g.sum()).to(a)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    m, terms = len(weights), []
    for j in range(m):
        n, c, h, w = a.shape
        assert min(h, w) >= WINDOW

        def win(t):
            t = t.reshape(n * c, 1, h, w)
            return F.conv2d(F.conv2d(t, g.view(1, 1, WINDOW, 1)), g.view(1, 1, 1, WINDOW))
        mu_a, mu_b = win(a), win(b)
        var_a, var_b, cov = win(a * a) - mu_a ** 2, win(b * b) - mu_b ** 2, win(a * b) - mu_a * mu_b
        cs = (2 * cov + c2) / (var_a + var_b + c2)
        lum = (2 * mu_a * mu_b + c1) / (mu_a ** 2 + mu_b ** 2 + c1)
        assert cs.shape[-2:] == (h - 10, w - 10)
        terms.append((lum * cs if j == m - 1 else cs).reshape(n, c, -1).mean(dim=2))
        if j < m - 1:
            a, b = F.avg_pool2d(a, 2), F.avg_pool2d(b, 2)
            assert a.shape[-2:] == (h // 2, w // 2)
    terms = torch.stack(terms)                                              # [M, N, C']
    positive = (terms > 0).all(dim=0)                                       # [N, C']
    wts = torch.tensor(weights, dtype=torch.float64).to(terms).view(m, 1, 1)
    powers = torch.where(positive.unsqueeze(0), terms, torch.ones_like(terms)) ** wts      # no fractional power of a term <= 0
    score = torch.where(positive, powers.prod(dim=0), torch.zeros_like(powers[0]))
    return score.mean(dim=1), terms


def _upstream(n):
    """a different upstream gradient for every image"""
    return 1.0 + 0.5 * torch.arange(n, dtype=torch.float64)


@functools.lru_cache(maxsize=None)
def _reference(shape, weights, crop, luma, dtype=torch.float64):
    """the definition on the CPU in `dtype` from the fp32 inputs -> (loss [N], terms [M, N, C'], da, db) for the upstream gradient
    _upstream(N) of the loss 1 - ms_ssim; never modified"""
    a, b = (t.to(dtype).requires_grad_() for t in _images(shape))
    ms, terms = _ms_definition(a, b, weights, crop_border=crop, luma=luma)
    loss = 1 - ms
    da, db = torch.autograd.grad((loss * _upstream(shape[0]).to(dtype)).sum(), (a, b))
    return loss.detach(), terms.detach(), da, db
