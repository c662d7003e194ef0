"""CPU: the host side of the resize of DESIGN.md section 27 -- argument checks before any HIP call, the tap table (the kernels' own
__host__ __device__ text) against torch's float64 operator, exact weights at ratio 2, and the mode draw's host restatement."""
import ctypes as C

import numpy as np
import pytest
import torch

from resize_cases import MODES, SHAPES, interp64, mats, noise, pkg, raw_taps

BADARG, TOOBIG, UNSUPPORTED = -1, -2, -3
P = 1 << 20                           # "pointers" that are never dereferenced: every call below is refused first
Q = 1 << 40


def _lib():
    return pkg('_lib').lib()


# ---- arguments ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fn', ['sisr_resize_fwd', 'sisr_resize_bwd'])
def test_kernel_entry_points_refuse_bad_arguments_before_any_hip_call(fn):
    f = getattr(_lib(), fn)
    good = [P, P + 4096, Q, 2, 3, 8, 8, 4, 4]              # src, modes, dst, N, C, H, W, h, w
    for k in (0, 1, 2):
        a = list(good)
        a[k] = None
        assert f(*a, None) == BADARG, k
    for k in range(3, 9):
        for v in (0, -1):
            a = list(good)
            a[k] = v
            assert f(*a, None) == BADARG, (k, v)
    a = list(good)
    a[2] = P + 64                                          # the output starts inside the input's bytes
    assert f(*a, None) == BADARG
    a = list(good)
    a[1] = Q + 4                                           # ... and the mode table inside the output's
    assert f(*a, None) == BADARG
    assert f(P, P + 4096, Q, 1, 1, 65536, 65536, 4, 4, None) == TOOBIG          # H W above INT32_MAX
    assert f(P, P + 4096, Q, 1, 1, 4, 4, 65536, 65536, None) == TOOBIG
    assert f(P, P + 4096, Q, 65536, 65536, 4, 4, 4, 4, None) == TOOBIG          # N C
    # not even a 1 x 1 tile fits: refused by both directions alike, down and up
    assert f(P, P + 4096, Q, 1, 1, 2000, 2000, 5, 5, None) == UNSUPPORTED
    assert f(P, P + 4096, Q, 1, 1, 5, 5, 2000, 2000, None) == UNSUPPORTED


def test_host_entry_points_refuse_bad_arguments():
    lib = _lib()
    first, count = np.zeros(8, np.int32), np.zeros(8, np.int32)
    w = np.zeros((8, pkg('_lib').RESIZE_MAX_TAPS), np.float32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)           # noqa: E731
    assert lib.sisr_resize_taps_host(2, 16, 8, ptr(first), ptr(count), ptr(w)) == 0
    for mode in (-1, 3):
        assert lib.sisr_resize_taps_host(mode, 16, 8, ptr(first), ptr(count), ptr(w)) == BADARG
    for n_in, n_out in ((0, 8), (16, 0), (-1, 8)):
        assert lib.sisr_resize_taps_host(1, n_in, n_out, ptr(first), ptr(count), ptr(w)) == BADARG
    for k in range(3):
        a = [ptr(first), ptr(count), ptr(w)]
        a[k] = None
        assert lib.sisr_resize_taps_host(1, 16, 8, *a) == BADARG
    assert lib.sisr_resize_taps_host(0, 8 * 65, 8, ptr(first), ptr(count), ptr(w)) == UNSUPPORTED      # an area window of 65
    assert lib.sisr_resize_taps_host(0, 8 * 64, 8, ptr(first), ptr(count), ptr(w)) == 0
    m = np.zeros(4, np.int32)
    assert lib.sisr_resize_modes_host(0, 1, 0, 4, 1.0, 1.0, 1.0, ptr(m)) == 0
    bad_p = [(-0.1, 0.5, 0.6), (0.0, 0.0, 0.0), (float('nan'), 0.5, 0.5), (float('inf'), 0.5, 0.5), (0.5, 0.5, -1e-9)]
    for p in bad_p:
        assert lib.sisr_resize_modes_host(0, 1, 0, 4, *p, ptr(m)) == BADARG, p
        assert lib.sisr_resize_modes_draw(P, 1, 0, 4, *p, Q, None) == BADARG, p
    assert lib.sisr_resize_modes_host(-1, 1, 0, 4, 1.0, 1.0, 1.0, ptr(m)) == BADARG
    assert lib.sisr_resize_modes_host(0, 1, 0, 4, 1.0, 1.0, 1.0, None) == BADARG
    for rank, B in ((-1, 4), (65536, 4), (0, 0)):
        assert lib.sisr_resize_modes_host(0, 1, rank, B, 1.0, 1.0, 1.0, ptr(m)) == BADARG
        assert lib.sisr_resize_modes_draw(P, 1, rank, B, 1.0, 1.0, 1.0, Q, None) == BADARG
    assert lib.sisr_resize_modes_draw(None, 1, 0, 4, 1.0, 1.0, 1.0, Q, None) == BADARG
    assert lib.sisr_resize_modes_draw(P, 1, 0, 4, 1.0, 1.0, 1.0, None, None) == BADARG


def test_python_surface_refuses_what_it_cannot_run():
    sisr, R = pkg(), pkg('resize')
    assert sisr.resize_taps is R.resize_taps and sisr.expected_resize_modes is R.expected_resize_modes and callable(sisr.resize)
    for fn in (R.resize, sisr.resize):                                     # the package's name is the callable module
        with pytest.raises(RuntimeError):
            fn(torch.zeros(1, 3, 8, 8), (4, 4))                            # a CPU tensor
    with pytest.raises(ValueError):
        R.resize(torch.zeros(1, 3, 8, 8, dtype=torch.float64), (4, 4))
    with pytest.raises(ValueError):
        R.resize(torch.zeros(3, 8, 8), (4, 4))
    with pytest.raises(ValueError):
        R.resize(torch.zeros(1, 3, 8, 8), (0, 4))
    with pytest.raises(ValueError):
        R.resize_taps('nearest', 8, 4)
    with pytest.raises(ValueError):
        R.resize_taps('area', 0, 4)
    with pytest.raises(ValueError):
        R.expected_resize_modes(0, 0, 4, (0, 0, 0))
    with pytest.raises(ValueError):
        R.expected_resize_modes(0, -1, 4, (1, 1, 1))


# ---- tap matrices ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('size_in,size_out', SHAPES)
def test_tap_matrices_are_torchs_operator(size_in, size_out, mode):
    """R_h x R_w^T against F.interpolate in float64: the weights are fp32, the expected difference about 1e-7"""
    Rh, Rw = mats(mode, size_in, size_out)
    x = noise((2, 3) + size_in, 5).to(torch.float64)
    ref = interp64(x, size_out, mode)
    err = float((Rh @ x @ Rw.T - ref).abs().max())
    bound = 1e-6 * float(x.abs().max())
    print('%s %s -> %s: max |R_h x R_w^T - torch| = %.3e (bound %.3e)' % (mode, size_in, size_out, err, bound))
    assert tuple(ref.shape[-2:]) == size_out and err <= bound
    for R in (Rh, Rw):
        assert float((R.sum(1) - 1).abs().max()) <= 1e-6


@pytest.mark.parametrize('size_in,size_out', SHAPES)
def test_area_weights_are_exactly_one_over_the_window(size_in, size_out):
    for n_in, n_out in zip(size_in, size_out):
        first, count, w = raw_taps('area', n_in, n_out)
        for o in range(n_out):
            s, e = (o * n_in) // n_out, -((-(o + 1) * n_in) // n_out)
            assert (int(first[o]), int(count[o])) == (s, e - s)
            assert (w[o, :e - s] == np.float32(1) / np.float32(e - s)).all() and (w[o, e - s:] == 0).all()


def test_unclamped_indices_of_the_border_rows():
    first, count, _ = raw_taps('bicubic', 5, 11)
    assert first[0] == -2 and first[-1] + count[-1] - 1 == 5 + 1 and (count == 4).all()      # i0 = -1 .. 4
    first, count, _ = raw_taps('bilinear', 5, 11)
    assert first[0] == 0 and first[-1] + count[-1] - 1 == 5 and (count == 2).all()


def test_weights_at_ratio_two_are_exact():
    for n_in in (16, 34):
        first, count, w = raw_taps('bilinear', n_in, n_in // 2)
        assert (first == 2 * np.arange(n_in // 2)).all() and (w[:, :2] == 0.5).all()
        first, count, w = raw_taps('bicubic', n_in, n_in // 2)
        assert (first == 2 * np.arange(n_in // 2) - 1).all()
        assert (w[:, :4] == np.array([-0.09375, 0.59375, 0.59375, -0.09375], np.float32)).all()
        first, count, w = raw_taps('area', n_in, n_in // 2)
        assert (count == 2).all() and (w[:, :2] == 0.5).all()


# ---- mode draw -------------------------------------------------------------------------------------------------------------------
def _draw_by_hand(seed, t, B, probs, rank):
    """the draw rebuilt from the numpy Philox on its counters: {t low, t high, b, 0xFE090000 | rank}, u0 = ((r0 >> 8) + 0.5) 2^-24,
    the weights divided by their fp32 sum, the first mode with p_i > 0 and u0 <= p_0 + .. + p_i"""
    f32 = np.float32
    r = pkg('draws').draw_words(seed, t, np.arange(B), 0xFE090000 | rank)
    u0 = ((r[:, 0] >> 8).astype(f32) + f32(0.5)) * f32(1.0 / 16777216.0)
    w = [f32(v) for v in probs]
    s = f32(f32(w[0] + w[1]) + w[2])
    p = [f32(v / s) for v in w]
    out = np.zeros(B, np.int32)
    for j in range(B):
        c, m = f32(0), 0
        for i in range(3):
            if p[i] > 0:
                m = i
            c = f32(c + p[i])
            if p[i] > 0 and u0[j] <= c:
                break
        out[j] = m
    return out


@pytest.mark.parametrize('probs', [(1 / 3, 1 / 3, 1 / 3), (0.5, 0.0, 0.5)])
def test_mode_frequencies(probs):
    R = pkg('resize')
    n = 16384
    m = R.expected_resize_modes(7, 3, n, probs)
    for i, p in enumerate(probs):
        share = float((m == i).mean())
        print('p = %.4f: drawn %.4f' % (p, share))
        if p == 0:
            assert not (m == i).any()
        assert abs(share - p) <= 5 * np.sqrt(p * (1 - p) / n)


def test_mode_draw_is_the_philox_restatement():
    R = pkg('resize')
    assert (R.expected_resize_modes(3, 0, 64, (0, 0, 1)) == 2).all()
    assert (R.expected_resize_modes(3, 0, 64, (0, 5.0, 0)) == 1).all()       # any positive sum
    for seed, t, B, probs, rank in ((1, 0, 37, (1 / 3, 1 / 3, 1 / 3), 0), ((1 << 40) + 5, (1 << 33) + 2, 64, (0.2, 0.3, 0.5), 7),
                                    (9, 11, 50, (2.0, 1.0, 1.0), 65535)):
        got = R.expected_resize_modes(seed, t, B, probs, rank)
        assert got.dtype == np.int32 and (got == _draw_by_hand(seed, t, B, probs, rank)).all()
        assert (got == R.expected_resize_modes(seed, t, B, probs, rank)).all()
    a, b = R.expected_resize_modes(1, 0, 256, (1, 1, 1)), R.expected_resize_modes(1, 1, 256, (1, 1, 1))
    assert (a != b).any()                                                    # the draw changes with the step ...
    assert (a != R.expected_resize_modes(1, 0, 256, (1, 1, 1), rank=1)).any() and (a != R.expected_resize_modes(2, 0, 256, (1, 1, 1))).any()
