"""The definitions, the inputs, the cases and the float64 references shared by test_artifact_cpu.py and test_gpu_artifact.py (a plain
module, not a conftest): the refined artifact map of the LDL loss (Liang et al., CVPR 2022), the L1 it weighs
and the gradients with the map held constant.  Everything here is float64 on the CPU unless a dtype is passed."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from filters_cases import F64, natural, noise, pkg, reflect  # noqa: F401

# (shape, K): each the smallest shape at which one thing can go wrong (tiles are 8 rows x 64 columns)
CASES = [
    ((1, 1, 4, 4), 7),            # H = P + 1: every window mirrors on both sides
    ((2, 3, 7, 5), 7),            # ragged, smaller than one tile; two patch weights
    ((1, 3, 4, 70), 7),           # minimal height, more than one tile column
    ((1, 3, 33, 65), 7),          # both axes cross a tile edge by one: ragged last tiles
    ((1, 1, 40, 131), 3),         # the smallest K
    ((1, 3, 37, 66), 11),         # the largest K
    ((2, 3, 96, 96), 7),          # a training size
]
AMPS = (0.05, 0.3)
IDS = [str(c).replace(' ', '') for c in CASES]

NEAR = 1e-6                       # |r_sr - r_ema| below which the fp32 roundings of the two residual sums may flip the mask (|values| <~ 1)
NEAR_SHARE = 1e-3                 # the share of such pixels a case may have
# MAP_BOUND: 8 x the largest distance of torch's own fp32 composition (reflect F.pad + unfold + torch.var) from float64 on these cases
# on a CPU, the convention of the filter tests: measured 4.2e-8 .. 1.223e-7 of the sample's largest map value away from near ties.
# LOSS_BOUND, relative: the fp32 composition L1Loss(m sr, m gt) is 6.2e-9 .. 2.2e-7 off (its products cancel), 8 x that would be
# 1.8e-6; the tighter 6e-7 is kept: 10 roundings of 2^-24, for the rounded map, the fp32 residual sums and the rounded result.
# test_artifact_cpu.py prints the distances of the fp32 composition and asserts that it stays inside both.
MAP_BOUND = 9.8e-7
LOSS_BOUND = 6e-7
GRAD_ROUNDINGS = 4 * 2.0 ** -24   # dsr against the float64 formula on the device's own map: kf, g kf, (g kf) m, each rounded once


def composition(gt, sr, ema, ksize, detach=True):
    """BasicSR's get_refined_artifact_map, line for line, in the dtype of its inputs -> [N, 1, H, W]"""
    residual_ema = torch.sum(torch.abs(gt - ema), 1, keepdim=True)
    residual_sr = torch.sum(torch.abs(gt - sr), 1, keepdim=True)
    patch_level_weight = torch.var(residual_sr.clone(), dim=(-1, -2, -3), keepdim=True) ** (1 / 5)
    pad = (ksize - 1) // 2
    residual_pad = F.pad(residual_sr.clone(), pad=[pad, pad, pad, pad], mode='reflect')
    unfolded = residual_pad.unfold(2, ksize, 1).unfold(3, ksize, 1)
    pixel_level_weight = torch.var(unfolded, dim=(-1, -2), unbiased=True, keepdim=True).squeeze(-1).squeeze(-1)
    overall_weight = patch_level_weight * pixel_level_weight
    overall_weight[residual_sr < residual_ema] = 0
    return overall_weight.detach() if detach else overall_weight


def composition_loss(sr, gt, m, weight=1.0):
    """BasicSR's L1Loss(m * sr, m * gt) per sample -> [N]"""
    return weight * (m * sr - m * gt).abs().mean(dim=(1, 2, 3))


def residuals64(gt, sr, ema):
    gt, sr, ema = gt.to(F64), sr.to(F64), ema.to(F64)
    return (gt - sr).abs().sum(1), (gt - ema).abs().sum(1)


def map64(gt, sr, ema, ksize, mask=None):
    """The independent restatement: explicit mirrored indices, the window's mean and then its squared deviations, tap by tap.
    -> (map [N, 1, H, W], masked [N, H, W] bool); `mask` (bool, True = zeroed) replaces the restatement's own when given"""
    r_sr, r_ema = residuals64(gt, sr, ema)
    n, h, w = r_sr.shape
    P = ksize // 2
    assert h > P and w > P
    ys = [torch.from_numpy(reflect(np.arange(h) + d - P, h)) for d in range(ksize)]
    xs = [torch.from_numpy(reflect(np.arange(w) + d - P, w)) for d in range(ksize)]
    taps = [r_sr[:, yi][:, :, xi] for yi in ys for xi in xs]
    mean = sum(taps) / (ksize * ksize)
    v = sum((t - mean) ** 2 for t in taps) / (ksize * ksize - 1)
    mu = r_sr.mean(dim=(1, 2), keepdim=True)
    p = (((r_sr - mu) ** 2).sum(dim=(1, 2), keepdim=True) / (h * w - 1)) ** 0.2
    own = r_sr < r_ema
    m = p * v
    m = torch.where(own if mask is None else mask, torch.zeros_like(m), m)
    return m.unsqueeze(1), own


def loss64(sr, gt, m, weight=1.0):
    """weight * mean_{c,y,x} m |sr - gt| -> [N]"""
    return weight * (m.to(F64) * (sr.to(F64) - gt.to(F64)).abs()).mean(dim=(1, 2, 3))


def grad64(sr, gt, m, g, weight=1.0):
    """dL/dsr of sum_n g[n] loss[n] with the map a constant: g[n] weight m sign(sr - gt) / (C H W); dL/dgt is its negative"""
    c, h, w = sr.shape[1:]
    return g.to(F64).view(-1, 1, 1, 1) * weight * m.to(F64) * torch.sign(sr.to(F64) - gt.to(F64)) / (c * h * w)


@functools.lru_cache(maxsize=None)
def inputs(shape, amp, seed=1):
    """-> (sr, gt, ema) fp32: a natural image, an output with grain and one ridge of error, an EMA output near it; never modified"""
    w = shape[-1]
    x = torch.arange(w, dtype=F64).view(1, 1, 1, w)
    gt = natural(shape, seed, 0.04)
    sr = (gt.to(F64) + 0.5 * noise(shape, seed + 1, amp).to(F64) + 0.5 * amp * torch.exp(-((x - 0.4 * w) / 3) ** 2)).to(torch.float32)
    ema = (sr.to(F64) + noise(shape, seed + 2, amp / 2).to(F64)).to(torch.float32)
    return sr, gt, ema


@functools.lru_cache(maxsize=None)
def case(shape, ksize, amp):
    """-> (sr, gt, ema, map64, masked64, near): near = the pixels whose mask the fp32 residual sums may flip; never modified"""
    sr, gt, ema = inputs(shape, amp)
    m, masked = map64(gt, sr, ema, ksize)
    r_sr, r_ema = residuals64(gt, sr, ema)
    return sr, gt, ema, m, masked, (r_sr - r_ema).abs() <= NEAR
