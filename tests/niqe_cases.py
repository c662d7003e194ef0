"""The definition, the cases, the inputs and the bounds shared by test_niqe_cpu.py and test_gpu_niqe.py (a plain module, not a
conftest): NIQE (Mittal, Soundararajan, Bovik, IEEE SPL 2013) as BasicSR's calculate_niqe computes it, restated from the formulas in
float64 NumPy (the steps are numbered as in include/sisr_hip.h).  Nothing here touches a GPU."""
import functools
import math
import os

import numpy as np
import torch

from filters_cases import F64, natural, noise, pkg  # noqa: F401

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'jpeg_pillow.npz')
NF = 36
STEP = 0.001
HALF_TAPS = np.array([-3, -9, 29, 111, 111, 29, -9, -3], np.float64) / 256.0
SHIFTS = ((0, 1), (1, 0), (1, 1), (1, -1))
ALPHA_COLS = np.array([0] + [2 + 4 * k for k in range(4)] + [18] + [20 + 4 * k for k in range(4)])       # the ten alphas of a row
OTHER_COLS = np.array([c for c in range(NF) if c not in set(ALPHA_COLS.tolist())])

# (name, shape, block, crop): each the smallest shape at which one thing can go wrong
CASES = [
    ('one_block', (1, 1, 16, 16), 16, 0),         # one block, every window touches the border, 8 x 8 at scale 2; the score is NaN (one row)
    ('fixture', (2, 3, 40, 52), 16, 0),           # luma + rint, the ragged remainder ignored (32 x 48: 6 blocks), two samples
    ('cropped', (1, 3, 34, 50), 16, 1),           # the crop view in front of the block crop
    ('block96', (1, 1, 96, 192), 96, 0),          # the default block: the largest LDS footprint
    ('constant', (1, 1, 64, 64), 32, 0),          # a block and its 3-pixel surround constant: alpha 0.2, NaNs, nanmean, the row left out
    ('noise', (1, 1, 64, 80), 16, 0),             # uniform noise: alpha at the table's last entry
    ('smooth', (1, 3, 160, 160), 32, 0),          # interior alphas
]
IDS = [c[0] for c in CASES]
VALUE_RANGE = (-1.0, 1.0)

# The bounds.  Nobody can derive them, so they are measured -- never against the code under test: the yardstick is this float64
# restatement against ITSELF with the MSCN planes of both scales rounded to fp32, the accuracy a cheaper kernel would have, on the
# cases above on a CPU (test_niqe_cpu.py prints the distances and asserts that they stay inside the bounds).  A feature's distance is
# taken relative to the largest magnitude of its column over the case's blocks (m, a difference of two betas, passes through 0), with
# both sides evaluated at the SAME alpha, so a step in alpha is not counted twice; the score's relative to the score.  8 x the largest,
# the convention of filters_cases.py and artifact_cases.py.
# measured: features 3.04e-8 .. 2.236e-6 (largest: 'one_block', whose columns hold one value each), scores under model_for 2.5e-9 ..
# 1.244e-6 (largest: 'cropped'); no fit of the 700 changes its table entry
FEATURE_BOUND = 1.7e-5
SCORE_BOUND = 9.9e-6
ALPHA_SHARE = 0.01                                # of a case's fits, rounded up to a whole fit, may differ by one table step
SCORE_ROUNDINGS = 2.0 ** -23                      # sisr_niqe_score on the device's own features: the fp32 result plus a double solve


@functools.lru_cache(maxsize=None)
def window():
    k = np.arange(-3, 4, dtype=np.float64)
    g = np.exp(-(k * k) / (2.0 * (7.0 / 6.0) ** 2))
    return g / g.sum()


@functools.lru_cache(maxsize=None)
def tables():
    """-> (alpha, G1, G2, G3, rho) float64 [9801]: alpha_j = 0.2 + 0.001 j, Gamma(k / alpha_j) by math.gamma"""
    alpha = 0.2 + STEP * np.arange(9801, dtype=np.float64)
    g1, g2, g3 = (np.array([math.gamma(k / float(a)) for a in alpha], np.float64) for k in (1.0, 2.0, 3.0))
    return alpha, g1, g2, g3, g2 * g2 / (g1 * g3)


# ---- steps 1 - 3 ---------------------------------------------------------------------------------------------------------------------
def plane64(img, block, crop=0, value_range=VALUE_RANGE):
    """step 1: fp32 [N, C, H, W] -> float64 [N, h1, w1]"""
    lo, hi = (float(np.float32(v)) for v in value_range)
    x = img.numpy().astype(np.float64)
    n, c, h, w = x.shape
    x = x[:, :, crop:h - crop, crop:w - crop]
    v = (x - lo) * (255.0 / (hi - lo))
    y = 16.0 + ((65.481 * v[:, 0] + 128.553 * v[:, 1]) + 24.966 * v[:, 2]) / 255.0 if c == 3 else v[:, 0]
    y = np.rint(y)
    return y[:, :y.shape[1] // block * block, :y.shape[2] // block * block]


def half_index(L):
    """-> [8, L / 2] the pixels out[i] reads: 2 i - 3 + k, mirrored with the edge pixel repeated"""
    j = 2 * np.arange(L // 2)[None, :] - 3 + np.arange(8)[:, None]
    j = np.where(j < 0, -j - 1, j)
    return np.where(j >= L, 2 * L - 1 - j, j)


def half64(p):
    """step 2: [N, h, w] -> [N, h / 2, w / 2], rows then columns"""
    iy, ix = half_index(p.shape[1]), half_index(p.shape[2])
    rows = sum(HALF_TAPS[k] * p[:, iy[k], :] for k in range(8))
    return sum(HALF_TAPS[k] * rows[:, :, ix[k]] for k in range(8))


def mscn64(p):
    """step 3 from the moments about the pixel -> (mscn, sigma), [N, h, w]"""
    g = window()
    n, h, w = p.shape
    pad = np.pad(p, ((0, 0), (3, 3), (3, 3)), mode='edge')
    m1, m2 = np.zeros_like(p), np.zeros_like(p)
    for dy in range(7):
        for dx in range(7):
            d = pad[:, dy:dy + h, dx:dx + w] - p
            wt = g[dy] * g[dx]
            m1 += wt * d
            m2 += wt * d * d
    sigma = np.sqrt(np.abs(m2 - m1 * m1))
    return -m1 / (sigma + 1.0), sigma


def mscn_raw64(p):
    """step 3 as upstream writes it, from the raw moments -> (mscn, sigma); for the CPU comparison only"""
    from scipy.ndimage import correlate1d
    g = window()
    blur = lambda a: correlate1d(correlate1d(a, g, axis=1, mode='nearest'), g, axis=2, mode='nearest')      # noqa: E731
    mu = blur(p)
    sigma = np.sqrt(np.abs(blur(p * p) - mu * mu))
    return (p - mu) / (sigma + 1.0), sigma


# ---- steps 4 - 5 ---------------------------------------------------------------------------------------------------------------------
def rhat64(f):
    """-> (L, R, Rhat) of a field"""
    f = f.reshape(-1)
    with np.errstate(all='ignore'):
        neg, pos = f[f < 0], f[f > 0]
        L = np.sqrt(np.float64((neg * neg).sum()) / np.float64(neg.size))
        R = np.sqrt(np.float64((pos * pos).sum()) / np.float64(pos.size))
        gam = L / R
        r = np.mean(np.abs(f)) ** 2 / np.mean(f * f)
        return L, R, r * (gam ** 3 + 1) * (gam + 1) / ((gam ** 2 + 1) ** 2)


def argmin_index(rhat):
    with np.errstate(all='ignore'):
        return int(np.argmin((tables()[4] - rhat) ** 2))


def search_index(rhat):
    """the kernel's search: the first j with rho_j >= Rhat, then the neighbour comparison; a NaN or an infinity: 0"""
    rho = tables()[4]
    if not abs(rhat) < math.inf:
        return 0
    lo = int(np.searchsorted(rho, rhat, side='left'))
    j = min(lo, len(rho) - 1)
    if 0 < lo < len(rho) and (rho[lo - 1] - rhat) ** 2 <= (rho[lo] - rhat) ** 2:
        j = lo - 1
    return j


def aggd64(f, j=None):
    """step 4 -> (j, (alpha, m, beta_l, beta_r)); `j` given: the formulas evaluated at that table entry"""
    alpha, g1, g2, g3, _ = tables()
    L, R, rhat = rhat64(f)
    if j is None:
        j = argmin_index(rhat)
    with np.errstate(all='ignore'):
        t = np.sqrt(g1[j] / g3[j])
        bl, br = L * t, R * t
        return j, (alpha[j], (br - bl) * (g2[j] / g1[j]), bl, br)


def block_features64(m, js=None):
    """step 5 for one block's MSCN at one scale -> ([18], the five table entries)"""
    out, used = [], []
    j, (a, _, bl, br) = aggd64(m, None if js is None else js[0])
    out += [a, (bl + br) / 2]
    used.append(j)
    for k, shift in enumerate(SHIFTS):
        j, fit = aggd64(m * np.roll(m, shift, axis=(0, 1)), None if js is None else js[1 + k])
        out += list(fit)
        used.append(j)
    return out, used


def features64(img, block, crop=0, value_range=VALUE_RANGE, js=None, round32=False):
    """steps 1 - 5 -> (feat [N, nb, 36], sharp [N, nb], js [N, nb, 10] int); `js` given: every fit evaluated at those table entries;
    round32: the MSCN planes of both scales rounded to fp32 (the yardstick of the bounds)"""
    p1 = plane64(img, block, crop, value_range)
    p2 = half64(p1)
    (m1, s1), (m2, _) = mscn64(p1), mscn64(p2)
    if round32:
        m1, m2 = (m.astype(np.float32).astype(np.float64) for m in (m1, m2))
    n, h, w = p1.shape
    nby, nbx = h // block, w // block
    feat = np.zeros((n, nby * nbx, NF))
    sharp = np.zeros((n, nby * nbx))
    used = np.zeros((n, nby * nbx, 10), np.int64)
    for i in range(n):
        for by in range(nby):
            for bx in range(nbx):
                b = by * nbx + bx
                row, ju = [], []
                for m, B in ((m1, block), (m2, block // 2)):
                    f, j = block_features64(m[i, by * B:(by + 1) * B, bx * B:(bx + 1) * B], None if js is None else js[i, b, len(ju):len(ju) + 5])
                    row += f
                    ju += j
                feat[i, b], used[i, b] = row, ju
                sharp[i, b] = s1[i, by * block:(by + 1) * block, bx * block:(bx + 1) * block].mean()
    return feat, sharp, used


def alpha_index(alpha):
    """the table entry behind an alpha"""
    return np.rint((np.asarray(alpha, np.float64) - 0.2) / STEP).astype(np.int64)


# ---- steps 6 - 7 ---------------------------------------------------------------------------------------------------------------------
def moments64(feat):
    """feat [nb, 36] -> (mu_d, cov_d, complete rows)"""
    import warnings
    with warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore')
        mu = np.nanmean(feat, axis=0)
        ok = feat[~np.isnan(feat).any(axis=1)]
        cov = np.cov(ok, rowvar=False) if ok.shape[0] >= 2 else np.full((NF, NF), np.nan)
    return mu, cov, ok.shape[0]


def score64(feat, mu_p, cov_p, pinv=False):
    """step 6 for one image -> float (NaN for fewer than two complete rows or an S that is not positive definite)"""
    mu, cov, rows = moments64(feat)
    S, d = (cov_p + cov) / 2, mu_p - mu
    if rows < 2 or np.isnan(S).any() or np.isnan(d).any():
        return math.nan
    if pinv:
        return float(np.sqrt(d @ np.linalg.pinv(S) @ d))
    try:
        c = np.linalg.cholesky(S)
    except np.linalg.LinAlgError:
        return math.nan
    y = np.linalg.solve(c, d)
    return float(np.sqrt(y @ y))


def select64(feat, sharp, sharpness=0.75):
    """step 7's rows of one batch: feat [N, nb, 36], sharp [N, nb] -> (keep [N, nb] bool, margin: the smallest relative distance of a
    sharpness from its image's threshold)"""
    thr = sharpness * sharp.max(axis=1, keepdims=True)
    keep = (sharp > thr) & ~np.isnan(feat).any(axis=2)
    return keep, float((np.abs(sharp - thr) / thr).min())


def fit64(rows):
    return rows.mean(axis=0), np.cov(rows, rowvar=False)


def model_for(feat):
    """a synthetic model near a case's own features, a function of the float64 restatement alone: S is positive definite whatever the
    rank of cov_d is, and cov_p is conditioned as a fitted model is (eigenvalues of its correlation part log-spaced over 1e-6 .. 1 on
    the DCT basis), so the score is as sensitive to the features as it is in use"""
    flat = feat.reshape(-1, NF)
    import warnings
    with warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore')
        mu = np.nan_to_num(np.nanmean(flat, axis=0), nan=1.0)
        sd = np.nan_to_num(np.nanstd(flat, axis=0), nan=0.0)
    scale = np.abs(mu) + sd + 0.05
    k = np.arange(NF)
    q = np.cos(np.pi * np.outer(k + 0.5, k) / NF) * np.sqrt(2.0 / NF)
    q[:, 0] /= np.sqrt(2.0)
    corr = (q * 10.0 ** (-6.0 * k / (NF - 1))) @ q.T
    return mu + 0.02 * scale * np.cos(k), corr * np.outer(scale, scale)


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
def smooth(shape, seed):
    """a natural image without the grain: shading, one edge, and texture far below the grey-level step"""
    n, c, h, w = shape
    y = torch.arange(h, dtype=F64).view(h, 1)
    x = torch.arange(w, dtype=F64).view(1, w)
    ripple = 0.12 * torch.sin(0.9 * x + 0.3 * y) * torch.cos(0.05 * x * (1 + 0.01 * y)) + 0.08 * torch.sin(0.37 * y - 0.21 * x)
    return (0.7 * natural(shape, seed, 0.03).to(F64) + ripple).to(torch.float32)


@functools.lru_cache(maxsize=None)
def image(name):
    """the input of a case, fp32 in (-1, 1); never modified"""
    shape = dict((c[0], c[1]) for c in CASES)[name]
    if name == 'fixture':
        img = torch.from_numpy(np.load(GOLDEN)['image'].astype(np.float32)) / 127.5 - 1            # [3, 40, 52]
        return torch.stack([img, img.flip(1) * 0.8 + 0.1 * noise(img.shape, 31, 1.0)])
    if name == 'constant':
        img = natural(shape, 32, 0.2)
        img[:, :, :35, :35] = 0.25
        return img
    if name == 'noise':
        return noise(shape, 33, 0.9)
    if name in ('block96', 'smooth'):
        return smooth(shape, 34)
    return natural(shape, 35 + len(name), 0.15)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (img fp32, block, crop, feat64 [N, nb, 36], sharp64 [N, nb], js [N, nb, 10]); never modified"""
    _, shape, block, crop = CASES[IDS.index(name)]
    img = image(name)
    assert tuple(img.shape) == shape
    return (img, block, crop) + features64(img, block, crop)


FIT_SHAPE, FIT_BLOCK = (4, 1, 160, 160), 32


def family(shape, seed):
    """planes of mixed sharpness: shading and an edge under grain that fades across the plane -> fp32 [N, 1, H, W]"""
    n, c, h, w = shape
    x = torch.arange(w, dtype=F64).view(1, 1, 1, w)
    y = torch.arange(h, dtype=F64).view(1, 1, h, 1)
    fade = 0.78 + 0.22 * torch.cos(0.02 * x + 0.013 * y + torch.arange(n, dtype=F64).view(n, 1, 1, 1) + seed)
    return (0.6 * natural(shape, seed, 0.0).to(F64) + 0.3 * fade * noise(shape, seed + 1, 1.0).to(F64)).to(torch.float32)


@functools.lru_cache(maxsize=None)
def fit_case():
    """four 160 x 160 planes -> (batches (two fp32 tensors of two planes), feat64, sharp64, keep, margin, (mu64, cov64)); never modified"""
    img = family(FIT_SHAPE, 41)
    feat, sharp, _ = features64(img, FIT_BLOCK)
    keep, margin = select64(feat, sharp)
    return (img[:2], img[2:]), feat, sharp, keep, margin, fit64(feat[keep])
