"""Writes tests/golden/draw_streams.npz: what every host twin of the device-side samplers returned at the commit BEFORE the draw
conventions moved into one place (csrc/sisr_philox.h, draws.py), recorded once so that tests/test_draw_streams_cpu.py can hold every
later commit to the same bits.  Recorded results only; ``streams()`` calls the package's host functions and nothing else.

  SISR_LIB=<the recording commit's libsisr_hip.so> python tests/golden/make_draw_streams_golden.py

``streams()`` -> {name: array}; the test calls it again and compares the raw bits, key for key.
"""
import ctypes as C
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = 'single-image-super-resolution_amd'
WIDE_SEED = (0xDEADBEEF << 32) | 0x1234567
WIDE_T = (5 << 32) + 77

# degrade.expected_params: seed, t, B, K, sigma, anisotropic, noise, rank
PARAMS = [(0, 0, 16, 21, (0.2, 3.0), True, (0.0, 0.1), 0), (WIDE_SEED, WIDE_T, 5, 7, (0.6, 5.0), False, (0.02, 0.02), 65535),
          (3, 9, 3, 1, (1.0, 1.0), True, (0.0, 0.0), 2), (77, 5, 5, 13, (0.2, 3.0), True, (0.01, 0.1), 4)]
# degrade.expected_mix with the final filter, B = 4, rank 3, t = 2^33 + i: family (None: the published mixture), K, ksize_min, blur_prob
MIX = [('iso', 7, 7, 1.0), ('aniso', 21, 7, 1.0), ('generalized_iso', 7, 3, 1.0), ('generalized_aniso', 5, 5, 1.0),
       ('plateau_iso', 7, 7, 0.5), ('plateau_aniso', 5, 1, 1.0), ('sinc', 21, 7, 1.0), (None, 21, 7, 0.8)]
FAMILIES = ('iso', 'aniso', 'generalized_iso', 'generalized_aniso', 'plateau_iso', 'plateau_aniso', 'sinc')
NOISE = dict(seed=0x9E3779B97F4A7C15, t=(1 << 33) + 5, first=6, count=1001, rank=7)
JPEG = [(0, 0, 0, 3, 30, 95), (WIDE_T, WIDE_SEED, 65535, 3, 1, 100)]                       # t, seed, rank, B, qlo, qhi
RESIZE_PROBS = [(1.0, 1.0, 1.0), (0.0, 2.0, 1.0), (0.0, 0.0, 1.0)]
PATCH = dict(seed=20240229, B=8, M=37, world=2, H0=11, W0=15, h=4, w=4, mask=7)            # epoch length 37 // (8 * 2) = 2


def _pkg(sub):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    return importlib.import_module(PKG + '.' + sub)


def _mix_stage(D, family, K, kmin, blur_prob):
    if family is None:
        return D.DegradeStage(ksize=K, ksize_min=kmin, blur_prob=blur_prob, noise=(2 / 255., 50 / 255.), shot=(0.05, 2.5))
    i = FAMILIES.index(family)
    probs = [0.0] * 6
    probs[i if i < 6 else 0] = 1.0
    return D.DegradeStage(ksize=K, ksize_min=kmin, blur_prob=blur_prob, kernel_probs=probs, sinc_prob=1.0 if i == 6 else 0.0,
                          noise=(0.0, 0.1), shot=(0.05, 3.0))


def streams():
    D, R, P, lib = _pkg('degrade'), _pkg('resize'), _pkg('patches'), _pkg('_lib').lib()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    out = {}
    for i, (seed, t, B, K, sigma, aniso, noise, rank) in enumerate(PARAMS):
        out['params%d_kernels' % i], out['params%d_sigma' % i], out['params%d_params' % i] = D.expected_params(seed, t, B, K, sigma, aniso, noise, rank)
    for i, (family, K, kmin, blur_prob) in enumerate(MIX):
        got = D.expected_mix(WIDE_SEED, (1 << 33) + i, 4, _mix_stage(D, family, K, kmin, blur_prob), rank=3, final_sinc_prob=0.5)
        for name, a in zip(('kernels', 'final', 'params', 'noise'), got):
            out['mix%d_%s' % (i, name)] = a
    for grey in (False, True):
        out['noise_grey' if grey else 'noise_colour'] = D.expected_noise(NOISE['seed'], NOISE['t'], NOISE['first'], NOISE['count'], NOISE['rank'], grey=grey)
    for i, (t, seed, rank, B, qlo, qhi) in enumerate(JPEG):
        q, tab = np.zeros(B, np.int32), np.zeros((B, 2, 8, 8), np.float32)
        assert lib.sisr_jpeg_tables_host(t, seed, rank, B, qlo, qhi, ptr(q), ptr(tab)) == 0
        out['jpeg%d_quality' % i], out['jpeg%d_tables' % i] = q, tab
    for i, probs in enumerate(RESIZE_PROBS):
        for rank in (0, 65535):
            out['resize%d_rank%d' % (i, rank)] = R.expected_resize_modes(WIDE_SEED, WIDE_T, 257, probs, rank)
    p = PATCH
    sizes = np.array([(p['h'] + i % 5, p['w'] + (3 * i) % 7) for i in range(p['M'])], dtype=np.int64)
    table = P.image_table(sizes, 3)[0]
    nb = p['M'] // (p['B'] * p['world'])
    for order, rank, t in ((o, r, t) for o in ('random', 'sequential', 'permuted') for r in range(p['world']) for t in (0, 4 * nb + 1)):
        head = (t, p['seed'], rank, p['world'], P.ORDERS[order], p['B'], p['M'])
        tail = (p['h'], p['w'], p['mask'])
        key = 'patch_%s_rank%d_t%d' % (order, rank, t)
        if order != 'permuted':                                   # the first entry point does not know the permuted order
            d = np.zeros((p['B'], 4), np.int32)
            assert lib.sisr_patch_draws_host(*head, p['H0'], p['W0'], *tail, ptr(d)) == 0
            out[key + '_first'] = d
        for name, tab, H0, W0 in (('uniform', None, p['H0'], p['W0']), ('table', table, 0, 0)):
            d = np.zeros((p['B'], 4), np.int32)
            assert lib.sisr_patch_draws_table_host(*head, H0, W0, None if tab is None else ptr(tab), *tail, ptr(d)) == 0
            out['%s_%s' % (key, name)] = d
    return out


if __name__ == '__main__':
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'draw_streams.npz')
    np.savez_compressed(path, **streams())
    print('wrote %s: %d bytes' % (path, os.path.getsize(path)))
