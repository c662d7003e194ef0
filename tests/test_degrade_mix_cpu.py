"""CPU: the host side of the second-order degradation: the new entry points refuse bad arguments before they
touch a GPU; the host restatement of the mixed draw (the device code's own text compiled for the host) equals the float64 formulas
of the seven kernel families, and its frequencies equal the settings' probabilities; the grey noise stream is its own."""
import ctypes as C

import numpy as np
import pytest

from degrade_mix_cases import FAMILIES, KERNEL_BOUND, forced_stage, j1, kernel_error, kernels64, pkg, support
from test_degrade_cpu import _uniforms

BADARG, TOOBIG = -1, -2
TAG_NOISE_GREY = 0xFE080000


def test_j1_reference_is_the_bessel_function():
    """the float64 reference itself: the series on [0, 6] (largest term 7: 1e-15 of cancellation) and three tabulated zeros"""
    x = np.linspace(0, 6, 61)
    k = np.arange(40, dtype=np.float64)
    fact = np.cumprod(np.concatenate([[1.0], np.arange(1, 41, dtype=np.float64)]))
    series = ((-1.0) ** k * (x[:, None] / 2) ** (2 * k + 1) / (fact[:40] * fact[1:41])).sum(axis=1)
    assert np.abs(j1(x) - series).max() <= 1e-14
    assert np.abs(j1(np.array([3.8317059702075125, 7.015586669815619, 41.61709421281445]))).max() <= 1e-14


@pytest.mark.parametrize('ksize_min_is_k', [False, True], ids=['kmin1', 'kminK'])
@pytest.mark.parametrize('K', [7, 21])
@pytest.mark.parametrize('family', FAMILIES)
def test_host_kernels_match_the_float64_formulas(family, K, ksize_min_is_k):
    D = pkg('degrade')
    stage = forced_stage(family, K, K if ksize_min_is_k else 1)
    k, fk, p, _ = D.expected_mix(0x5EED0000 + K, 3, 128, stage, rank=1, final_sinc_prob=0.5)
    fam = FAMILIES.index(family)
    assert (p[:, 0] == fam).all() and (p[:, 7] == 1).all()
    if ksize_min_is_k:
        assert (p[:, 1] == K).all()
    else:
        assert set(p[:, 1].astype(int)) == set(range(1, K + 1, 2))           # 128 draws over at most 11 sizes
    err = kernel_error(k, p, K)
    print('%s K %d: max err / largest weight %.3e' % (family, K, err))
    assert err <= KERNEL_BOUND
    assert (k[~support(p, K)] == 0).all()
    assert np.abs(k.astype(np.float64).sum(axis=(1, 2)) - 1).max() <= 1e-6
    if fam == 6 and K == 21:
        assert (k < 0).any()                                                  # the sinc kernel's negative lobes
    # iso forms: one sigma, no rotation; only the generalised / plateau forms carry a beta, only sinc a cutoff
    if fam in (0, 2, 4, 6):
        assert np.array_equal(p[:, 2], p[:, 3]) and (p[:, 4] == 0).all()
    else:
        assert (p[:, 2] != p[:, 3]).all() and (p[:, 4] > 0).all()
    assert ((p[:, 5] > 0) == (fam in (2, 3, 4, 5))).all() and ((p[:, 6] > 0) == (fam == 6)).all()
    # the final filter: sinc or delta, on its own support
    centre = np.zeros((K, K), np.float32)
    centre[K // 2, K // 2] = 1
    is_delta = (fk == centre).all(axis=(1, 2))
    assert is_delta.any() and (K == 1 or not is_delta.all())
    assert np.abs(fk.astype(np.float64).sum(axis=(1, 2)) - 1).max() <= 1e-6


def test_blur_off_is_exactly_the_delta_kernel():
    D = pkg('degrade')
    for K in (1, 7, 21):
        k, fk, p, _ = D.expected_mix(4, 0, 16, D.DegradeStage(ksize=K, ksize_min=1, blur_prob=0.0), final_sinc_prob=0.0)
        want = np.zeros((16, K, K), np.float32)
        want[:, K // 2, K // 2] = 1
        assert (p[:, 7] == 0).all() and np.array_equal(k, want) and np.array_equal(fk, want)
        assert np.array_equal(kernels64(p, K), want.astype(np.float64))
    assert D.expected_mix(4, 0, 2, D.DegradeStage())[1] is None               # no final filter asked for


def _within(count, n, prob):
    return abs(count / n - prob) <= 5 * np.sqrt(prob * (1 - prob) / n)


def test_draw_frequencies_and_ranges_over_16384_host_draws():
    D = pkg('degrade')
    n, K, kmin = 16384, 15, 7
    st = D.DegradeStage(ksize=K, ksize_min=kmin, blur_prob=0.8, sinc_prob=0.1, sigma=(0.2, 1.5), noise=(2 / 255., 50 / 255.),
                        shot=(0.05, 2.5), gaussian_prob=0.5, grey_prob=0.4)
    _, fk, p, nt = D.expected_mix(20240229, 17, n, st, rank=3, final_sinc_prob=0.8)
    fam, k_eff = p[:, 0].astype(int), p[:, 1].astype(int)
    probs = [(1 - st.sinc_prob) * q for q in st.kernel_probs] + [st.sinc_prob]
    for i, q in enumerate(probs):
        print('family %-18s %.4f (%.4f)' % (FAMILIES[i], (fam == i).mean(), q))
        assert _within((fam == i).sum(), n, q), FAMILIES[i]
    sizes = list(range(kmin, K + 1, 2))
    assert set(k_eff) == set(sizes)
    for s in sizes:
        assert _within((k_eff == s).sum(), n, 1 / len(sizes)), s
    assert _within((p[:, 7] == 1).sum(), n, st.blur_prob)
    assert set(nt[:, 0]) == {1.0, 2.0} and (nt[:, 3] == 0).all()
    assert _within((nt[:, 0] == 1).sum(), n, st.gaussian_prob)
    assert _within((nt[:, 1] == 1).sum(), n, st.grey_prob) and set(nt[:, 1]) == {0.0, 1.0}
    centre = np.zeros((K, K), np.float32)
    centre[K // 2, K // 2] = 1
    assert _within((~(fk == centre).all(axis=(1, 2))).sum(), n, 0.8)
    # every drawn parameter inside its range
    f32 = np.float32
    for col in (2, 3):
        assert (p[:, col] >= f32(st.sigma[0])).all() and (p[:, col] <= f32(st.sigma[1])).all()
    assert (p[:, 4] >= 0).all() and (p[:, 4] <= f32(np.pi)).all()
    gen, plat, sinc = (fam == 2) | (fam == 3), (fam == 4) | (fam == 5), fam == 6
    assert (p[gen, 5] >= f32(st.beta_gaussian[0])).all() and (p[gen, 5] <= f32(st.beta_gaussian[1])).all()
    assert (p[plat, 5] >= f32(st.beta_plateau[0])).all() and (p[plat, 5] <= f32(st.beta_plateau[1])).all()
    assert (p[~(gen | plat), 5] == 0).all() and (p[~sinc, 6] == 0).all()
    small = sinc & (k_eff < 13)
    assert small.any() and (sinc & ~small).any()
    assert (p[small, 6] >= f32(np.pi / 3)).all() and (p[sinc, 6] >= f32(np.pi / 5)).all() and (p[sinc, 6] <= f32(np.pi)).all()
    assert (p[sinc & ~small, 6] < f32(np.pi / 3)).any()                        # the wider range is really used from 13 on
    g, s = nt[:, 0] == 1, nt[:, 0] == 2
    assert (nt[g, 2] >= f32(st.noise[0])).all() and (nt[g, 2] <= f32(st.noise[1])).all()
    assert (nt[s, 2] >= f32(st.shot[0])).all() and (nt[s, 2] <= f32(st.shot[1])).all()
    # the draw is a pure function of (seed, t, b, rank)
    again = D.expected_mix(20240229, 17, 8, st, rank=3, final_sinc_prob=0.8)
    assert np.array_equal(again[2], p[:8]) and np.array_equal(again[3], nt[:8]) and np.array_equal(again[1], fk[:8])
    for other in (D.expected_mix(20240229, 18, 8, st, rank=3), D.expected_mix(20240229, 17, 8, st, rank=4), D.expected_mix(1, 17, 8, st, rank=3)):
        assert not np.array_equal(other[2], p[:8])
    none = D.expected_mix(1, 0, 8, D.DegradeStage(noise=(0, 0), shot=(0, 0)))[3]
    assert (none == 0).all()                                                   # both ranges (0, 0): mode none


def test_grey_noise_is_its_own_deterministic_stream_and_colour_is_the_existing_one():
    D, lib = pkg('degrade'), pkg('_lib').lib()
    seed, t, rank, first, count = 0x9E3779B97F4A7C15, (1 << 33) + 5, 7, 6, 1001
    grey, colour = D.expected_noise(seed, t, first, count, rank, grey=True), D.expected_noise(seed, t, first, count, rank)
    assert np.array_equal(grey, D.expected_noise(seed, t, first, count, rank, grey=True))
    assert not np.array_equal(grey, colour) and np.abs(grey - colour).max() > 1
    direct = np.zeros(count, np.float32)
    assert lib.sisr_degrade_noise_host(t, seed, rank, first, count, direct.ctypes.data_as(C.c_void_p)) == 0
    assert np.array_equal(colour, direct) and np.array_equal(colour, D.expected_noise(seed, t, first, count, rank, grey=False))
    # the grey stream is Box-Muller on the counters tagged 0xFE08, as the colour stream is on 0xFE02
    e = np.arange(first, first + count)
    u = _uniforms(seed, t, e // 4, TAG_NOISE_GREY, rank)
    pair, rows = np.where(e % 4 < 2, 0, 2), np.arange(count)
    ang = 2 * np.pi * u[rows, pair + 1]
    z64 = np.sqrt(-2 * np.log(u[rows, pair])) * np.where(e % 2 == 1, np.sin(ang), np.cos(ang))
    assert np.abs(grey - z64).max() <= 2e-5
    assert abs(float(grey.mean())) < 5 / np.sqrt(count) and abs(float(grey.var()) - 1) < 5 * np.sqrt(2 / count)


def _mix(**kw):
    L = pkg('_lib')
    base = dict(K=21, ksize_min=7, blur_prob=1.0, sinc_prob=0.1, kernel_probs=(0.45, 0.25, 0.12, 0.03, 0.12, 0.03), sigma_lo=0.2,
                sigma_hi=3.0, beta_g_lo=0.5, beta_g_hi=4.0, beta_p_lo=1.0, beta_p_hi=2.0, noise_lo=0.0, noise_hi=0.1, shot_lo=0.05,
                shot_hi=3.0, gaussian_prob=0.5, grey_prob=0.4, final_sinc_prob=0.8)
    base.update(kw)
    base['kernel_probs'] = (C.c_float * 6)(*base['kernel_probs'])
    return L.DegradeMix(**base)


def test_every_bad_argument_is_refused_without_a_gpu():
    L = pkg('_lib')
    lib = L.lib()
    assert lib.sisr_degrade_mix_bytes() == C.sizeof(L.DegradeMix)
    buf = (C.c_float * (2 * 21 * 21 + 64))()
    p = C.cast(buf, C.c_void_p)             # a non-null pointer: refused calls never read it, and nothing here reaches a launch
    nan = float('nan')
    bad_mixes = [dict(K=0), dict(K=4), dict(K=23), dict(K=-1), dict(ksize_min=0), dict(ksize_min=8), dict(ksize_min=23), dict(K=7, ksize_min=9),
                 dict(blur_prob=-0.1), dict(blur_prob=1.1), dict(sinc_prob=2.0), dict(sinc_prob=nan), dict(gaussian_prob=-1.0),
                 dict(grey_prob=1.5), dict(final_sinc_prob=-0.5), dict(final_sinc_prob=nan),
                 dict(kernel_probs=(0.5, 0.25, 0.12, 0.03, 0.12, 0.03)), dict(kernel_probs=(0.4, 0.25, 0.12, 0.03, 0.12, 0.03)),
                 dict(kernel_probs=(1.2, -0.2, 0, 0, 0, 0)), dict(kernel_probs=(nan, 0, 0, 0, 0, 0)), dict(kernel_probs=(0,) * 6),
                 dict(sigma_lo=3.5), dict(sigma_lo=0.0), dict(sigma_lo=-1.0), dict(sigma_hi=nan), dict(beta_g_lo=5.0), dict(beta_g_lo=0.0),
                 dict(beta_p_lo=2.5), dict(beta_p_hi=float('inf')), dict(noise_lo=-0.1), dict(noise_lo=0.2), dict(shot_lo=4.0),
                 dict(shot_lo=-1.0), dict(shot_hi=nan)]
    good_draw = dict(step=p, seed=1, rank=0, B=2, mix=C.byref(_mix()), k=p, fk=p, params=p, nt=p, t=p, stream=None)
    good_host = dict(t=0, seed=1, rank=0, B=2, mix=C.byref(_mix()), k=p, fk=None, params=p, nt=p)
    assert lib.sisr_degrade_mix_host(*good_host.values()) == 0
    assert lib.sisr_degrade_mix_host(*dict(good_host, fk=p).values()) == 0
    for bad in bad_mixes:
        m = C.byref(_mix(**bad))
        assert lib.sisr_degrade_draw_mix(*dict(good_draw, mix=m).values()) == BADARG, bad
        assert lib.sisr_degrade_mix_host(*dict(good_host, mix=m).values()) == BADARG, bad
    for bad in (dict(step=None), dict(mix=None), dict(k=None), dict(params=None), dict(nt=None), dict(t=None), dict(B=0), dict(B=-3),
                dict(rank=-1), dict(rank=65536)):
        assert lib.sisr_degrade_draw_mix(*dict(good_draw, **bad).values()) == BADARG, bad
    for bad in (dict(mix=None), dict(k=None), dict(params=None), dict(nt=None), dict(t=-1), dict(B=0), dict(rank=-1), dict(rank=65536)):
        assert lib.sisr_degrade_mix_host(*dict(good_host, **bad).values()) == BADARG, bad
    good_fwd = dict(x=p, table=p, step=p, seed=1, rank=0, y=p, N=1, C=3, h=4, w=4, clamp=1, stream=None)
    for bad in (dict(x=None), dict(table=None), dict(step=None), dict(y=None), dict(N=0), dict(C=0), dict(C=5), dict(h=0), dict(w=0),
                dict(rank=-1), dict(rank=65536)):
        assert lib.sisr_degrade_noise_fwd(*dict(good_fwd, **bad).values()) == BADARG, bad
    assert lib.sisr_degrade_noise_fwd(*dict(good_fwd, N=1 << 14, C=4, h=1 << 9, w=1 << 9).values()) == TOOBIG      # N C h w = 2^34
    good_bwd = dict(dy=p, y=None, dx=p, N=1, C=3, h=4, w=4, stream=None)
    for bad in (dict(dy=None), dict(dx=None), dict(N=0), dict(C=0), dict(C=5), dict(h=0), dict(w=0)):
        assert lib.sisr_degrade_noise_bwd(*dict(good_bwd, **bad).values()) == BADARG, bad
    assert lib.sisr_degrade_noise_bwd(*dict(good_bwd, N=1 << 14, C=4, h=1 << 9, w=1 << 9).values()) == TOOBIG
    for bad in (dict(z=None), dict(t=-1), dict(rank=-1), dict(rank=65536), dict(first=-1), dict(count=0)):
        a = dict(dict(t=0, seed=1, rank=0, first=0, count=4, z=p), **bad)
        assert lib.sisr_degrade_noise_grey_host(*a.values()) == BADARG, bad
    assert lib.sisr_degrade_noise_grey_host(0, 1, 0, (1 << 34) - 2, 3, p) == TOOBIG


def test_python_surface_validates_and_refuses_a_cpu_device():
    import torch
    D = pkg('degrade')
    for bad in (dict(ksize=4), dict(ksize=23), dict(ksize_min=4), dict(ksize=7, ksize_min=9), dict(blur_prob=1.5), dict(sinc_prob=-0.1),
                dict(kernel_probs=(0.5, 0.5)), dict(kernel_probs=(0.5, 0.25, 0.12, 0.03, 0.12, 0.03)), dict(kernel_probs=(1.5, -0.5, 0, 0, 0, 0)),
                dict(sigma=(0., 1.)), dict(sigma=(2., 1.)), dict(beta_gaussian=(0., 1.)), dict(beta_plateau=(2., 1.)), dict(noise=(-1., 0.)),
                dict(noise=(1., 0.)), dict(shot=(3., 1.)), dict(gaussian_prob=2.0), dict(grey_prob=-1.0), dict(jpeg=(0, 50)),
                dict(jpeg=(60, 50)), dict(jpeg=(50, 101))):
        with pytest.raises(ValueError):
            D.DegradeStage(**bad)
    s1, s2 = D.realesrgan_stages()
    assert (s1.blur_prob, s2.blur_prob, s1.sigma, s2.sigma) == (1.0, 0.8, (0.2, 3.0), (0.2, 1.5))
    assert np.allclose(s1.noise, (2 / 255, 60 / 255)) and np.allclose(s2.noise, (2 / 255, 50 / 255))
    assert (s1.shot, s2.shot, s1.jpeg, s2.jpeg) == ((0.05, 3.0), (0.05, 2.5), (30, 95), (30, 95))
    assert (s1.ksize, s1.ksize_min, s1.sinc_prob, s1.gaussian_prob, s1.grey_prob) == (21, 7, 0.1, 0.5, 0.4)
    for bad in (dict(stages=()), dict(stages=('x',)), dict(mid_size=(0, 4)), dict(mid_size=(4, 4), mid_scale=(0.3, 0.7)),
                dict(mid_scale=(0.0, 1.0)), dict(mid_scale=(0.8, 0.4)), dict(final_sinc_prob=1.5), dict(final_order='random'),
                dict(jpeg_subsampling='422'), dict(jpeg_grad='none'), dict(rank=65536), dict(seed=-1)):
        with pytest.raises(ValueError):
            D.HighOrderDegrader(**bad)
    with pytest.raises(RuntimeError):
        D.HighOrderDegrader(device='cpu')
    with pytest.raises(RuntimeError):
        D.degrade_noise(torch.zeros(1, 3, 4, 4), torch.zeros(1, 4), 0)         # a CPU tensor: no fallback
    with pytest.raises(ValueError):
        D.expected_mix(0, -1, 2, s1)
    with pytest.raises(ValueError):
        D.expected_mix(0, 0, 2, s1, final_sinc_prob=1.5)
