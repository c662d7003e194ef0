"""The definition, the cases and the float64 reference shared by test_freq_loss_cpu.py and test_gpu_freq_loss.py (a plain module,
not a conftest).  Inputs: image_cases._images / _view.

The definition is written with torch ops in the dtype of its inputs, on the crop / luma view [N, C', H', W']:

    'l1' / 'charbonnier' (BasicSR's FFTLoss):  D = rfft2(a) - rfft2(b), unnormalised;
                                               loss[n] = mean over (C', kh, kw < W' // 2 + 1, {Re, Im}) of |z| / sqrt(z^2 + eps^2)
    'focal' (Jiang et al., ICCV 2021; patch_factor 1, no log_matrix / ave_spectrum / batch_matrix):
                                               D = fft2(a, norm='ortho') - fft2(b, norm='ortho'), dist = |D|^2,
                                               w = sqrt(dist)^alpha / max_{kh,kw}(...) per (n, plane), NaN -> 0, clamped to [0, 1],
                                               detached;  loss[n] = mean_{C',kh,kw}(w dist)

`closed_form_focal` is the half-spectrum form the kernels evaluate: per plane sum_k h_k |D_k|^(2 + alpha) / (max|D|^alpha (H' W')^2)
with D unnormalised and Hermitian weights h_k = 1 for kw = 0 and (W' even) kw = W' / 2, otherwise 2."""
import functools

import torch

from image_cases import _images, _view

KINDS = ('l1', 'charbonnier', 'focal')

# (shape, crop, luma): each the smallest shape at which one thing can go wrong
CASES = [
    ((1, 1, 1, 1), 0, False),            # DC alone
    ((1, 1, 2, 2), 0, False),            # every bin structurally real: exact-zero Im, the gradient of L1 equal in every pixel
    ((2, 1, 4, 6), 0, False),            # both sides even: Nyquist row and column; two images with different upstream gradients
    ((2, 3, 7, 9), 0, False),            # odd / even mixes: Wh, the Hermitian weights, no Nyquist column when W' is odd
    ((2, 3, 8, 9), 0, False),
    ((2, 3, 9, 8), 0, False),
    ((2, 3, 17, 33), 0, False),          # one past a power of two and past two 8-line blocks: ragged row / column blocks
    ((2, 3, 21, 36), 2, True),           # the view: offset on load, luma transpose in the backward, zero border
    ((1, 3, 45, 70), 1, False),          # ragged blocks in both axes
    ((1, 3, 96, 96), 4, True),           # the training sizes: several blocks per axis, the longest sums
    ((1, 3, 96, 192), 0, False),
    ((1, 1, 192, 192), 0, False),
]
# the cases whose L1 GRADIENT is compared: the sign margin condition holds (test_freq_loss_cpu.py asserts it).  On the others the
# smallest |Re D| / |Im D| over thousands of bins comes too close to 0 for a sign to be safe in fp32, and one flipped sign moves
# the whole gradient by about 2 / sqrt(count): they compare the L1 value only and take their gradient checks from 'charbonnier'
# and 'focal', which run the same backward kernels
L1_GRAD_CASES = [((1, 1, 1, 1), 0, False), ((1, 1, 2, 2), 0, False), ((2, 1, 4, 6), 0, False), ((2, 3, 7, 9), 0, False),
                 ((2, 3, 8, 9), 0, False), ((2, 3, 9, 8), 0, False), ((2, 3, 21, 36), 2, True)]
SIGN_MARGIN = 1e-4


def defn(a, b, kind, crop=0, luma=False, alpha=1.0, eps=1e-3):
    """the loss as torch ops in the dtype of a and b -> (loss [N], D); differentiable"""
    a, b = _view(a, crop, luma), _view(b, crop, luma)
    if kind in ('l1', 'charbonnier'):
        D = torch.fft.rfft2(a) - torch.fft.rfft2(b)
        z = torch.stack([D.real, D.imag], -1)
        rho = z.abs() if kind == 'l1' else torch.sqrt(z * z + eps * eps)
        return rho.mean(dim=(1, 2, 3, 4)), D
    assert kind == 'focal'
    D = torch.fft.fft2(a, norm='ortho') - torch.fft.fft2(b, norm='ortho')
    dist = D.real ** 2 + D.imag ** 2
    wt = torch.sqrt(dist) ** alpha
    wt = wt / wt.amax(dim=(2, 3), keepdim=True)
    wt = torch.nan_to_num(wt, nan=0.0).clamp(0, 1).detach()
    return (wt * dist).mean(dim=(1, 2, 3)), D


def closed_form_focal(a, b, crop=0, luma=False, alpha=1.0):
    """the focal loss from the unnormalised HALF spectrum with Hermitian weights -> loss [N]; an all-zero plane contributes 0"""
    a, b = _view(a, crop, luma), _view(b, crop, luma)
    n, c, h, w = a.shape
    D = torch.fft.rfft2(a - b)
    mag = D.abs()
    hk = torch.full((w // 2 + 1,), 2.0, dtype=a.dtype)
    hk[0] = 1.0
    if w % 2 == 0:
        hk[w // 2] = 1.0
    mx = mag.amax(dim=(2, 3))
    s = (hk * mag ** (2.0 + alpha)).sum(dim=(2, 3))
    per_plane = torch.where(mx > 0, s / (mx.clamp_min(1e-300) ** alpha * float(h * w) ** 2), torch.zeros_like(s))
    return per_plane.mean(dim=1)


def upstream(n, dtype=torch.float64):
    """a different upstream gradient for every image"""
    return (1.0 + 0.5 * torch.arange(n, dtype=torch.float64)).to(dtype)


def evaluate(shape, crop, luma, kind, dtype, alpha=1.0, eps=1e-3, seed=0):
    """the definition in `dtype` on the CPU -> (loss [N], da, db, D) for the upstream gradient 1 + 0.5 n"""
    a, b = (t.to(dtype).requires_grad_() for t in _images(shape, seed))
    loss, D = defn(a, b, kind, crop, luma, alpha, eps)
    da, db = torch.autograd.grad((loss * upstream(shape[0], dtype)).sum(), (a, b))
    return loss.detach(), da, db, D.detach()


@functools.lru_cache(maxsize=None)
def _reference(shape, crop, luma, kind, alpha=1.0, eps=1e-3):
    """float64 on the CPU -> (loss [N], da, db, D); never modified"""
    return evaluate(shape, crop, luma, kind, torch.float64, alpha, eps)


def structural_imag_zero(h, w):
    """[h, w // 2 + 1] bool: the bins of the half spectrum whose imaginary part is zero for every real input"""
    m = torch.zeros(h, w // 2 + 1, dtype=torch.bool)
    rows = [0] + ([h // 2] if h % 2 == 0 else [])
    cols = [0] + ([w // 2] if w % 2 == 0 else [])
    for r in rows:
        for c in cols:
            m[r, c] = True
    return m
