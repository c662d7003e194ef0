"""GPU: NIQE (csrc/niqe.hip, metrics.niqe / niqe_features / NiqeModel) against the float64 restatement of
niqe_cases.py, through the C entry points (guards around every output and the workspace, two launches with identical bits) and
through the Python surface.

Bounds (niqe_cases.py).  Every device alpha lies within one table step of the restatement's, and at most 1 % of a case's fits,
rounded up to a whole fit, may differ at all.  Every other feature is compared with the restatement's formula evaluated AT THE
DEVICE'S alpha, relative to the largest magnitude of its column over the case's blocks, within FEATURE_BOUND = 1.7e-5: 8 x the
largest distance (2.236e-6) of the restatement from itself with its MSCN planes rounded to fp32, measured on a CPU.  NaN positions
are equal exactly.  The score: sisr_niqe_score on the device's own features against the float64 formula within 2^-23 relative (the
fp32 result plus a double solve), and end to end within SCORE_BOUND = 9.9e-6 relative (8 x 1.244e-6, the same yardstick)."""
import math

import numpy as np
import pytest
import torch

import niqe_cases as K
from niqe_cases import IDS, pkg
from gpu_helpers import Buf, run2

pytestmark = pytest.mark.gpu
F64 = torch.float64


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _features_entry(img, block, crop, with_sharp=True):
    """-> (feat [N, nb, 36] float64, sharp [N, nb] fp32 or None) on the CPU through sisr_niqe_features, launched twice: status 0, guards of
    the features, the sharpness and the workspace intact, identical bits"""
    M, lib = pkg('metrics'), pkg('_lib').lib()
    n, c, h, w = img.shape
    nb = ((h - 2 * crop) // block) * ((w - 2 * crop) // block)
    size = lib.sisr_niqe_ws_bytes(n, h, w, crop, block)
    assert size > 0 and size % 8 == 0
    ws, feat, sharp = Buf(size // 8, dtype=F64), Buf(n * nb * 36, dtype=F64), Buf(n * nb)
    tables, x = M._niqe_tables(torch.device('cuda', torch.cuda.current_device())), img.cuda()
    call = lambda: lib.sisr_niqe_features(x.data_ptr(), n, c, h, w, crop, K.VALUE_RANGE[0], K.VALUE_RANGE[1], block, tables.data_ptr(),   # noqa: E731
                                          ws.ptr(), feat.ptr(), sharp.ptr() if with_sharp else None, _stream())
    run2(call, [feat, sharp, ws])
    if not with_sharp:
        assert bool((sharp.body == sharp.fill).all())
    return feat.cpu().view(n, nb, 36).numpy().copy(), sharp.cpu().view(n, nb).numpy().copy() if with_sharp else None


def _reference_at(name, got):
    """the alphas of the device against the restatement's (the step rule), then the restatement evaluated at the device's alphas"""
    img, block, crop, feat64, sharp64, js = K.case(name)
    alpha = got[..., K.ALPHA_COLS]
    assert not np.isnan(alpha).any()
    j_dev = K.alpha_index(alpha)
    assert np.abs(alpha - K.tables()[0][j_dev]).max() <= 1e-12, 'an alpha that is no table entry'
    moved = int((j_dev != js).sum())
    print('%s: %d of %d fits differ from the restatement (at most %d may, by one step)' % (name, moved, js.size, math.ceil(K.ALPHA_SHARE * js.size)))
    assert int(np.abs(j_dev - js).max()) <= 1 and moved <= math.ceil(K.ALPHA_SHARE * js.size)
    return (feat64 if moved == 0 else K.features64(img, block, crop, js=j_dev)[0]), sharp64


def _check_features(name, got, ref):
    assert np.array_equal(np.isnan(got), np.isnan(ref)), 'NaN positions differ'
    oc = K.OTHER_COLS
    with np.errstate(all='ignore'):
        mag = np.nanmax(np.abs(ref[..., oc]).reshape(-1, len(oc)), axis=0)
        err = np.abs(got[..., oc] - ref[..., oc]) / mag
    worst = float(np.nanmax(err))
    print('%s: max |f - f64| / max |column| %.3e (bound %.1e)' % (name, worst, K.FEATURE_BOUND))
    assert worst <= K.FEATURE_BOUND


def _model(mu, cov, block):
    return pkg('metrics').NiqeModel(mu, cov, block).to('cuda')


@pytest.mark.parametrize('name', IDS)
def test_features_and_score_match_float64(name):
    M, lib = pkg('metrics'), pkg('_lib').lib()
    img, block, crop, feat64 = K.case(name)[:4]
    got, sharp = _features_entry(img, block, crop)
    ref, sharp64 = _reference_at(name, got)
    _check_features(name, got, ref)
    rel = float(np.abs(sharp.astype(np.float64) - sharp64).max() / sharp64.max())
    print('%s: sharpness %.3e of the largest (bound 2^-23)' % (name, rel))
    assert rel <= 2.0 ** -23
    # the Python surface: the same bits, with and without the sharpness
    f_py, s_py = M.niqe_features(img.cuda(), block, crop, return_sharpness=True)
    only = M.niqe_features(img.cuda(), block, crop)
    assert f_py.dtype == F64 and s_py.dtype == torch.float32 and f_py.shape == got.shape and s_py.shape == sharp.shape
    assert np.array_equal(f_py.cpu().numpy(), got, equal_nan=True) and np.array_equal(s_py.cpu().numpy(), sharp)
    assert np.array_equal(only.cpu().numpy(), got, equal_nan=True)
    assert np.array_equal(_features_entry(img, block, crop, with_sharp=False)[0], got, equal_nan=True)
    # ---- the score: the entry point on the device's own features, then end to end
    mu_p, cov_p = K.model_for(feat64)
    model = _model(mu_p, cov_p, block)
    n, nb = got.shape[:2]
    fd, score, ws = f_py.contiguous(), Buf(n), Buf(max(n * nb, 2), dtype=torch.int32, fill=7)
    call = lambda: lib.sisr_niqe_score(fd.data_ptr(), n, nb, model.mu.data_ptr(), model.cov.data_ptr(), ws.ptr(), score.ptr(), _stream())      # noqa: E731
    run2(call, [score, ws])
    s_dev = score.cpu().numpy().astype(np.float64)
    s_own = np.array([K.score64(got[i], mu_p, cov_p) for i in range(n)])
    s_ref = np.array([K.score64(feat64[i], mu_p, cov_p) for i in range(n)])
    end = M.niqe(img.cuda(), model, crop_border=crop)
    assert end.dtype == torch.float32 and end.shape == (n,) and np.array_equal(end.cpu().numpy().astype(np.float64), s_dev, equal_nan=True)
    print('%s: score %s; on the own features %s, restatement %s' % (name, s_dev.tolist(), s_own.tolist(), s_ref.tolist()))
    if name == 'one_block':
        assert np.isnan(s_dev).all() and np.isnan(s_ref).all()
        return
    d_own, d_ref = float((np.abs(s_dev - s_own) / s_own).max()), float((np.abs(s_dev - s_ref) / s_ref).max())
    print('%s: relative to the formula on the own features %.3e (bound %.3e), end to end %.3e (bound %.1e)'
          % (name, d_own, K.SCORE_ROUNDINGS, d_ref, K.SCORE_BOUND))
    assert d_own <= K.SCORE_ROUNDINGS and d_ref <= K.SCORE_BOUND


def test_a_model_that_makes_s_indefinite_gives_nan_and_a_batch_equals_separate_calls():
    M = pkg('metrics')
    img = torch.cat([K.noise((1, 1, 64, 80), 50 + i, 0.9 - 0.2 * i) for i in range(3)]).cuda()
    feat = K.features64(img.cpu(), 16)[0]
    assert not np.isnan(feat).any()
    mu_p, cov_p = K.model_for(feat)
    model = _model(mu_p, cov_p, 16)
    batch = M.niqe(img, model)
    one = torch.cat([M.niqe(img[i:i + 1], model) for i in range(3)])
    print('batch %s' % batch.tolist())
    assert torch.equal(batch, one) and bool(torch.isfinite(batch).all()) and len(set(batch.tolist())) == 3
    assert torch.equal(M.niqe(img, model), batch)                                      # two calls: equal bits
    bad = M.niqe(img, _model(mu_p, -1e6 * np.eye(36), 16))
    assert bool(torch.isnan(bad).all())
    # a strided input is made contiguous; the value range is applied
    wide = torch.zeros(3, 1, 64, 160, device='cuda')
    wide[..., ::2] = img
    assert torch.equal(M.niqe(wide[..., ::2], model), batch)
    assert torch.equal(M.niqe(2 * img, model, value_range=(-2.0, 2.0)), batch)          # 2 (x + 1) 63.75 is (x + 1) 127.5, rounded once


def test_niqe_is_capturable():
    """torch.cuda.graph captures niqe on a side stream with the image a static input; replays on new contents are bit-equal to eager
    calls on those contents"""
    M = pkg('metrics')
    name = 'fixture'
    img, block, crop, feat64 = K.case(name)[:4]
    model = _model(*K.model_for(feat64), block)
    static = torch.zeros(img.shape, device='cuda')
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            M.niqe(static + 0.1, model)                                                # uploads the tables, raises the LDS cap
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = M.niqe(static, model)
    for rep in range(3):
        x = (img.flip(3) if rep == 1 else img.roll(5 * rep, 2)).contiguous().cuda()
        static.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        eager = M.niqe(x, model)
        assert torch.equal(out, eager) and bool(torch.isfinite(out).all()), rep


def test_fit_selects_the_restatements_blocks_and_matches_its_moments():
    M = pkg('metrics')
    batches, feat64, sharp64, keep64, margin, _ = K.fit_case()
    assert margin > 1e-6 and keep64.sum() >= 37
    dev = [b.cuda() for b in batches]
    model = M.NiqeModel.fit(dev, block=K.FIT_BLOCK)
    assert model.block == K.FIT_BLOCK and model.mu.dtype == F64 and model.mu.is_cuda and tuple(model.cov.shape) == (36, 36)
    got = [M.niqe_features(b, K.FIT_BLOCK, return_sharpness=True) for b in dev]
    feat = torch.cat([g[0] for g in got]).cpu().numpy()
    sharp = torch.cat([g[1] for g in got]).cpu().numpy().astype(np.float64)
    keep, _ = K.select64(feat, sharp)
    print('fit: %d of %d rows kept (restatement %d), margin %.2e' % (keep.sum(), keep.size, keep64.sum(), margin))
    assert np.array_equal(keep, keep64)
    j_dev, js = K.alpha_index(feat[..., K.ALPHA_COLS]), K.alpha_index(feat64[..., K.ALPHA_COLS])
    moved = int((j_dev != js).sum())
    assert int(np.abs(j_dev - js).max()) <= 1 and moved <= math.ceil(K.ALPHA_SHARE * js.size)
    ref = feat64 if moved == 0 else K.features64(torch.cat(batches), K.FIT_BLOCK, js=j_dev)[0]
    mu64, cov64 = K.fit64(ref[keep64])
    # a feature moves by at most FEATURE_BOUND of its column's magnitude, so a mean does too, and a covariance -- a mean of products of
    # two deviations, each at most twice the magnitude -- by at most 4 FEATURE_BOUND of the product of the two magnitudes
    mag = np.abs(ref[keep64]).max(axis=0)
    d_mu = float((np.abs(model.mu.cpu().numpy() - mu64) / mag).max())
    d_cov = float((np.abs(model.cov.cpu().numpy() - cov64) / np.outer(mag, mag)).max())
    print('fit: mu %.3e (bound %.1e), cov %.3e (bound %.1e)' % (d_mu, K.FEATURE_BOUND, d_cov, 4 * K.FEATURE_BOUND))
    assert d_mu <= K.FEATURE_BOUND and d_cov <= 4 * K.FEATURE_BOUND
    with pytest.raises(ValueError, match='feature rows'):
        M.NiqeModel.fit(dev[:1], block=K.FIT_BLOCK, sharpness=0.97)


def test_evaluation_entry_points_add_the_score_only_when_asked():
    M, U, ut = pkg('metrics'), pkg('upscale'), pkg('utils')
    torch.manual_seed(5)
    net = pkg('model_generator').Generator(1, 16, 64, [2], use_sn=True).cuda().train()
    hr = (torch.rand(2, 3, 40, 40, generator=torch.Generator().manual_seed(6)) * 2 - 1).cuda()
    model = _model(*K.model_for(K.case('fixture')[3]), 16)
    plain = M.evaluate_generator(net, hr, (20, 20))
    out = M.evaluate_generator(net, hr, (20, 20), niqe_model=model)
    assert sorted(plain) == ['psnr', 'ssim'] and sorted(out) == ['niqe', 'psnr', 'ssim']
    assert torch.equal(out['psnr'], plain['psnr']) and torch.equal(out['ssim'], plain['ssim'])
    net.eval()
    with torch.no_grad():
        sr = net(ut.lr_from_hr(hr, (20, 20)))
    net.train()
    assert torch.equal(out['niqe'], M.niqe(sr, model, crop_border=2)) and bool(torch.isfinite(out['niqe']).all())

    class Recorded:
        """what evaluate_image uses of an Upscaler, keeping the SR image it scored"""

        def __init__(self, up):
            self.up, self.scale, self.mean, self.std = up, up.scale, up.mean, up.std

        def __call__(self, x):
            self.sr = self.up(x)
            return self.sr
    up = Recorded(U.Upscaler(net, tile=32))
    img = (torch.rand(40, 48, 3, generator=torch.Generator().manual_seed(7)) * 255).to(torch.uint8).cuda()
    plain = U.evaluate_image(up, img)
    out = U.evaluate_image(up, img, niqe_model=model)
    assert sorted(plain) == ['psnr', 'ssim'] and sorted(out) == ['niqe', 'psnr', 'ssim']
    assert torch.equal(out['psnr'], plain['psnr']) and torch.equal(out['ssim'], plain['ssim'])
    assert torch.equal(out['niqe'], M.niqe(up.sr[None], model, crop_border=2)) and out['niqe'].shape == (1,)
    assert bool(torch.isfinite(out['niqe']).all())
