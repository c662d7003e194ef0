"""CPU: the host side of NIQE: the float64 restatement of niqe_cases.py against scipy's filters and the dyadic
down-scaling weights; the table and the search the kernel uses against the argmin of the definition; Cholesky against the
pseudo-inverse; the score's order on a blurred and a noisy copy; the yardstick distances the bounds of the GPU test are taken from;
the new entry points refuse every bad argument before they touch a GPU; the Python surface validates, saves and loads."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import niqe_cases as K
from niqe_cases import IDS, pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BADARG, TOOBIG, UNSUPPORTED = -1, -2, -3


def test_window_and_downscale_are_what_the_definition_states():
    from scipy.ndimage import correlate1d
    g = K.window()
    assert abs(g.sum() - 1) < 1e-15 and np.array_equal(g, g[::-1]) and abs(g[3] / g[2] - math.exp(0.5 / (7 / 6) ** 2)) < 1e-14
    p = K.plane64(K.image('cropped'), 16, 1)
    # moments about the pixel against the raw moments through scipy's replicated border: the same MSCN to the digits the raw form keeps
    (m, s), (mr, sr) = K.mscn64(p), K.mscn_raw64(p)
    print('mscn: about the pixel - raw moments %.3e, sigma %.3e' % (np.abs(m - mr).max(), np.abs(s - sr).max()))
    assert np.abs(m - mr).max() < 1e-9 and np.abs(s - sr).max() < 1e-8
    mu = correlate1d(correlate1d(p, g, axis=1, mode='nearest'), g, axis=2, mode='nearest')
    pad = np.pad(p, ((0, 0), (3, 3), (3, 3)), mode='edge')
    direct = sum(g[a] * g[b] * pad[:, a:a + p.shape[1], b:b + p.shape[2]] for a in range(7) for b in range(7))
    assert np.abs(mu - direct).max() < 1e-11
    # the dyadic weights are 0.5 cubic(-0.5) at the distances 1.75, 1.25, 0.75, 0.25
    cubic = lambda x: (1.5 * x ** 3 - 2.5 * x ** 2 + 1) if x <= 1 else (-0.5 * x ** 3 + 2.5 * x ** 2 - 4 * x + 2)      # noqa: E731
    assert np.array_equal(K.HALF_TAPS, np.array([0.5 * cubic(0.5 * abs(k - 3.5)) for k in range(8)])) and K.HALF_TAPS.sum() == 1.0
    assert K.half_index(16)[:, 0].tolist() == [2, 1, 0, 0, 1, 2, 3, 4] and K.half_index(16)[:, 7].tolist() == [11, 12, 13, 14, 15, 15, 14, 13]
    const = np.full((1, 16, 32), 77.0)
    assert np.array_equal(K.half64(const), np.full((1, 8, 16), 77.0))
    ramp = np.arange(32, dtype=np.float64)[None, None, :].repeat(16, 1)
    assert np.array_equal(K.half64(ramp)[0, 3, 2:14], 2 * np.arange(2, 14) + 0.5)          # a ramp is sampled at the half-pixel centres
    h = K.half64(p)
    assert h.shape == (1, 16, 24) and np.array_equal(h * 65536, np.rint(h * 65536))        # exact: multiples of 2^-16


def test_table_is_monotone_and_the_search_is_the_argmin():
    alpha, g1, g2, g3, rho = K.tables()
    d = np.diff(rho)
    print('rho: %.6f .. %.6f, steps %.2e .. %.2e' % (rho[0], rho[-1], d.min(), d.max()))
    assert len(alpha) == 9801 and alpha[0] == 0.2 and abs(alpha[-1] - 10.0) < 1e-12 and d.min() > 1e-6
    lib_tables = pkg('metrics').niqe_tables_host()
    assert lib_tables.shape == (4, 9801) and all(np.array_equal(a, b) for a, b in zip(lib_tables, (g1, g2, g3, rho)))
    rng = np.random.default_rng(5)
    probes = np.concatenate([rng.uniform(rho[0] - 0.05, rho[-1] + 0.05, 4000), rho[rng.integers(0, 9801, 200)],
                             0.5 * (rho[:-1] + rho[1:])[rng.integers(0, 9800, 200)], [math.nan, math.inf, -math.inf, -1.0, 0.0, 5.0, rho[0], rho[-1]]])
    for r in probes:
        assert K.search_index(r) == K.argmin_index(r), r
    assert K.search_index(math.nan) == 0 and K.search_index(5.0) == 9800 and K.search_index(-1.0) == 0


@pytest.mark.parametrize('name', IDS)
def test_yardstick_distances_stay_inside_the_bounds(name):
    """what the GPU test's bounds are taken from, and the conditions its cases stand on"""
    img, block, crop, feat, sharp, js = K.case(name)
    f32, _, j32 = K.features64(img, block, crop, round32=True)
    at = K.features64(img, block, crop, js=j32)[0]
    assert np.array_equal(np.isnan(f32), np.isnan(at))
    oc = K.OTHER_COLS
    with np.errstate(all='ignore'):
        mag = np.nanmax(np.abs(at[..., oc]).reshape(-1, len(oc)), axis=0)
        d_feat = float(np.nanmax(np.abs(f32[..., oc] - at[..., oc]) / mag))
    mu_p, cov_p = K.model_for(feat)
    scores = [(K.score64(feat[i], mu_p, cov_p), K.score64(f32[i], mu_p, cov_p)) for i in range(feat.shape[0])]
    d_score = max((abs(a - b) / a for a, b in scores if a == a), default=0.0)
    moved = int((js != j32).sum())
    print('%s: %d fits, %d move under fp32 MSCN planes; feature distance %.3e (bound %.1e), score distance %.3e (bound %.1e); alpha %.3f .. '
          '%.3f, %d NaNs, scores %s' % (name, js.size, moved, d_feat, K.FEATURE_BOUND, d_score, K.SCORE_BOUND, np.nanmin(feat[..., K.ALPHA_COLS]),
                                        np.nanmax(feat[..., K.ALPHA_COLS]), int(np.isnan(feat).sum()), [a for a, _ in scores]))
    assert d_feat <= K.FEATURE_BOUND and d_score <= K.SCORE_BOUND
    assert moved <= math.ceil(K.ALPHA_SHARE * js.size) and int(np.abs(js - j32).max()) <= 1
    if name == 'one_block':
        assert feat.shape[1] == 1 and math.isnan(scores[0][0])
    else:
        assert all(a > 0 for a, _ in scores)
    if name == 'constant':                      # block 0 at scale 1: alpha 0.2 and NaNs; scale 2 reaches past the constant surround
        assert np.array_equal(np.isnan(feat[0, 0]), np.isin(np.arange(36), K.OTHER_COLS) & (np.arange(36) < 18))
        assert np.all(feat[0, 0, K.ALPHA_COLS[:5]] == 0.2) and not np.isnan(feat[0, 1:]).any() and sharp[0, 0] == 0.0
    else:
        assert not np.isnan(feat).any()
    if name == 'noise':
        assert (js[..., :5] == 9800).any()
    if name == 'smooth':
        assert js.min() > 100 and js.max() < 9000


def test_cholesky_is_the_pseudo_inverse_and_degraded_copies_score_higher():
    from scipy.ndimage import gaussian_filter
    _, feat, _, keep, margin, (mu_p, cov_p) = K.fit_case()
    print('fit: %d of %d rows kept, margin from the threshold %.2e, cond(cov) %.2e' % (keep.sum(), keep.size, margin, np.linalg.cond(cov_p)))
    assert keep.sum() >= 37 and margin > 1e-6
    img = K.family((1, 1, 160, 160), 77)
    blurred = torch.from_numpy(gaussian_filter(img.numpy().astype(np.float64), (0, 0, 1.5, 1.5))).float()
    noisy = (img + K.noise(img.shape, 78, 0.35)).clamp(-1, 1)
    got = []
    for x in (img, blurred, noisy):
        f = K.features64(x, K.FIT_BLOCK)[0][0]
        a, b = K.score64(f, mu_p, cov_p), K.score64(f, mu_p, cov_p, pinv=True)
        assert abs(a - b) <= 1e-7 * a, (a, b)
        got.append(a)
    print('scores under the family model: image %.9f, blurred %.9f, noisy %.9f' % tuple(got))
    assert got[0] < got[1] and got[0] < got[2]
    assert math.isnan(K.score64(feat[0], mu_p, -1e6 * np.eye(36)))


def test_header_binding_and_library_agree_and_refuse_bad_arguments_without_a_gpu():
    Lb = pkg('_lib')
    lib = Lb.lib()
    hdr = open(os.path.join(ROOT, 'include', 'sisr_hip.h')).read()
    for name in ('sisr_niqe_ws_bytes', 'sisr_niqe_features', 'sisr_niqe_score'):
        assert re.search(r'\b%s\s*\(' % name, hdr) and name in Lb.EXPORTS and hasattr(lib, name)
    for macro, value in (('SISR_NIQE_MAX_BLOCK', Lb.NIQE_MAX_BLOCK), ('SISR_NIQE_FEATURES', Lb.NIQE_FEATURES), ('SISR_NIQE_TABLE', Lb.NIQE_TABLE)):
        assert re.search(r'#define %s %d\b' % (macro, value), hdr)
    # ---- the size query: the two planes in double and one flag per block
    assert lib.sisr_niqe_ws_bytes(2, 40, 52, 0, 16) == 8 * (2 * 32 * 48 + 2 * 16 * 24) + 4 * 2 * 6
    assert lib.sisr_niqe_ws_bytes(1, 34, 50, 1, 16) == 8 * (32 * 48 * 5 // 4) + 8 * 3
    for bad in ((0, 40, 40, 0, 16), (1, 0, 40, 0, 16), (1, 40, -1, 0, 16), (1, 40, 40, -1, 16), (1, 40, 40, 0, 17), (1, 40, 40, 0, 14),
                (1, 200, 200, 0, 98), (1, 40, 40, 0, 0)):
        assert lib.sisr_niqe_ws_bytes(*bad) == BADARG, bad
    for bad in ((1, 15, 40, 0, 16), (1, 40, 40, 13, 16), (1, 95, 200, 0, 96)):
        assert lib.sisr_niqe_ws_bytes(*bad) == UNSUPPORTED, bad
    assert lib.sisr_niqe_ws_bytes(1, 1 << 16, 1 << 16, 0, 16) == TOOBIG and lib.sisr_niqe_ws_bytes(1 << 20, 1 << 10, 1 << 10, 0, 16) == TOOBIG
    # ---- refused calls never read their pointers and reach no launch: non-null, 8-byte aligned values 16 MiB apart
    buf = (C.c_double * 8)()
    p = C.cast(buf, C.c_void_p)
    q, r, s, t = (C.c_void_p(p.value + (i << 24)) for i in (1, 2, 3, 4))
    nan, inf = float('nan'), float('inf')
    good = dict(img=p, N=2, C=3, H=40, W=52, crop=0, lo=-1.0, hi=1.0, block=16, tables=q, ws=r, feat=s, sharp=t, stream=None)
    for bad in (dict(img=None), dict(tables=None), dict(ws=None), dict(feat=None), dict(ws=C.c_void_p(r.value + 4)), dict(feat=C.c_void_p(s.value + 4)),
                dict(N=0), dict(N=-1), dict(H=0), dict(W=-3), dict(crop=-1), dict(block=15), dict(block=14), dict(block=98), dict(block=0),
                dict(lo=nan), dict(hi=inf), dict(lo=1.0, hi=1.0), dict(lo=1.0, hi=-1.0)):
        assert lib.sisr_niqe_features(*dict(good, **bad).values()) == BADARG, bad
    for bad in (dict(C=0), dict(C=2), dict(C=4), dict(H=15), dict(crop=13), dict(block=96)):
        assert lib.sisr_niqe_features(*dict(good, **bad).values()) == UNSUPPORTED, bad
    for bad in (dict(H=1 << 16, W=1 << 16), dict(N=1 << 20, H=1 << 10, W=1 << 10), dict(N=70000, H=16, W=16, C=1)):
        assert lib.sisr_niqe_features(*dict(good, **bad).values()) == TOOBIG, bad
    good = dict(feat=p, N=2, nb=6, mu=q, cov=r, ws=s, score=t, stream=None)
    for bad in (dict(feat=None), dict(mu=None), dict(cov=None), dict(ws=None), dict(score=None), dict(N=0), dict(nb=0), dict(nb=-1),
                dict(ws=C.c_void_p(s.value + 4)), dict(mu=C.c_void_p(q.value + 4))):
        assert lib.sisr_niqe_score(*dict(good, **bad).values()) == BADARG, bad
    assert lib.sisr_niqe_score(*dict(good, N=1 << 20, nb=1 << 10).values()) == TOOBIG


def test_python_surface_validates_before_the_device_check():
    M, top = pkg('metrics'), pkg()
    assert top.niqe is M.niqe and top.niqe_features is M.niqe_features and top.NiqeModel is M.NiqeModel
    model = M.NiqeModel(np.zeros(36), np.eye(36), block=16)
    x = torch.zeros(2, 3, 40, 52)
    calls = (lambda a, **kw: M.niqe_features(a, **dict(dict(block=16), **kw)), lambda a, **kw: M.niqe(a, model, **kw),
             lambda a, **kw: M.NiqeModel.fit([a], **dict(dict(block=16), **kw)))
    for call in calls:
        with pytest.raises(RuntimeError):
            call(x)                                                # a legal call on a CPU tensor: no fallback
        with pytest.raises(RuntimeError):
            call(x.transpose(2, 3))                                # strided is legal (made contiguous); CPU is not
        for bad in (x.double(), x.half(), x.to(torch.bfloat16), None, x[0], x[:, :2], torch.zeros(0, 3, 40, 52), torch.zeros(1, 3, 15, 52)):
            with pytest.raises(ValueError):
                call(bad)
        for bad in (-1, 1.0, True, None, 13):                      # 13: 14 x 26 remain
            with pytest.raises(ValueError):
                call(x, crop_border=bad)
        for bad in ((1.0, 1.0), (1.0, -1.0), (0.0, float('inf')), (float('nan'), 1.0), 2.0, (0.0, 1.0, 2.0), None):
            with pytest.raises(ValueError):
                call(x, value_range=bad)
    for bad in (15, 14, 98, 0, 16.0, True, None):
        with pytest.raises(ValueError):
            M.niqe_features(x, block=bad)
        with pytest.raises(ValueError):
            M.NiqeModel.fit([x], block=bad)
        with pytest.raises(ValueError):
            M.NiqeModel(np.zeros(36), np.eye(36), block=bad)
    for bad in (1.0, -0.1, float('nan'), None, True):
        with pytest.raises(ValueError):
            M.NiqeModel.fit([x], block=16, sharpness=bad)
    with pytest.raises(ValueError):
        M.NiqeModel.fit([], block=16)
    with pytest.raises(ValueError):
        M.niqe(x, (np.zeros(36), np.eye(36)))
    with pytest.raises(ValueError):
        M.niqe(torch.zeros(1, 3, 40, 52), M.NiqeModel(np.zeros(36), np.eye(36)))        # the model's block, 96, does not fit
    for mu, cov in ((np.zeros(35), np.eye(36)), (np.zeros(36), np.eye(35)), (np.zeros((2, 36)), np.eye(36)), (np.zeros(36), np.zeros((36, 37)))):
        with pytest.raises(ValueError):
            M.NiqeModel(mu, cov)


def test_model_files_round_trip_and_upstream_style_files_load(tmp_path):
    M = pkg('metrics')
    rng = np.random.default_rng(3)
    mu, a = rng.normal(size=36), rng.normal(size=(36, 36))
    model = M.NiqeModel(mu, a @ a.T, block=32)
    assert model.mu.dtype == torch.float64 and model.cov.dtype == torch.float64 and model.block == 32
    path = str(tmp_path / 'model.npz')
    model.save(path)
    with np.load(path) as z:
        assert sorted(z.files) == ['block', 'cov_pris_param', 'mu_pris_param'] and z['mu_pris_param'].shape == (1, 36)
    back = M.NiqeModel.load(path)
    assert torch.equal(back.mu, model.mu) and torch.equal(back.cov, model.cov) and back.block == 32
    moved = back.to('cpu')
    assert moved is not back and torch.equal(moved.cov, back.cov) and moved.block == 32
    upstream = str(tmp_path / 'niqe_pris_params.npz')                                   # [1, 36] means, no block entry
    np.savez(upstream, mu_pris_param=mu[None], cov_pris_param=a @ a.T)
    up = M.NiqeModel.load(upstream)
    assert up.block == 96 and tuple(up.mu.shape) == (36,) and torch.equal(up.mu, model.mu)
    np.savez(str(tmp_path / 'other.npz'), mu=mu)
    with pytest.raises(ValueError):
        M.NiqeModel.load(str(tmp_path / 'other.npz'))


def test_evaluation_entry_points_take_a_model_and_tools_parse():
    import importlib.util
    import inspect
    M, U = pkg('metrics'), pkg('upscale')
    assert inspect.signature(M.evaluate_generator).parameters['niqe_model'].default is None
    assert inspect.signature(U.evaluate_image).parameters['niqe_model'].default is None
    for tool in ('upscale_image', 'fit_niqe'):
        spec = importlib.util.spec_from_file_location(tool, os.path.join(ROOT, 'tools', tool + '.py'))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        if tool == 'upscale_image':
            assert mod.parse_args(['c.pt', 'a.png', 'b.png']).niqe is None
            assert mod.parse_args(['c.pt', 'a.png', 'b.png', '--niqe', 'm.npz']).niqe == 'm.npz'
        else:
            a = mod.parse_args(['dir', 'out.npz'])
            assert (a.block, a.sharpness, a.crop_border) == (96, 0.75, 0)
            with pytest.raises(SystemExit):
                mod.parse_args(['dir', 'out.npz', '--block', '15'])
