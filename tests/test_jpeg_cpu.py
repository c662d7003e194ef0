"""CPU: the host side of the JPEG round trip.  The tables are libjpeg's (a Pillow recording under
tests/golden/); the quality draw's host text agrees with the documented Philox counter; a float64 restatement of the definition,
written here and imported by the GPU tests, is JPEG apart from the decoder's integer transforms (compared with Pillow's decoded
images); every entry point refuses bad arguments before it touches a GPU."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

PKG = 'single-image-super-resolution_amd'
BADARG, TOOBIG = -1, -2
TAG_QUALITY = 0xFE030000
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'jpeg_pillow.npz')


def pkg(sub):
    return importlib.import_module(PKG + '.' + sub)


def golden():
    return np.load(GOLDEN)


# ---- the float64 restatement ----------------------------------------------------------------------------------------------------
COLOUR = torch.tensor([[0.299, 0.587, 0.114], [-0.168735892, -0.331264108, 0.5], [0.5, -0.418687589, -0.081312411]], dtype=torch.float64)
COLOUR_INV = torch.linalg.inv(COLOUR)
_k, _n = torch.meshgrid(torch.arange(8, dtype=torch.float64), torch.arange(8, dtype=torch.float64), indexing='ij')
DCT = torch.cos((2 * _n + 1) * _k * np.pi / 16) * 0.5
DCT[0] = np.sqrt(1 / 8)


def mcu_of(C, sub):
    return 16 if (sub == '420' and C == 3) else 8


def _blocks(plane):
    n, h, w = plane.shape
    return plane.reshape(n, h // 8, 8, w // 8, 8).permute(0, 1, 3, 2, 4)


def _unblocks(b):
    n, by, bx = b.shape[:3]
    return b.permute(0, 1, 3, 2, 4).reshape(n, by * 8, bx * 8)


def jpeg64(x, tables, sub='444', clamp=True, grad='ste', detail=False):
    """The definition of sisr_hip.h in float64 torch ops, differentiable: x [N, C, H, W], tables [N, 2, 8, 8].  The rounding is
    round(u).detach() plus the surrogate's differentiable part.  detail: also the list of u per plane ([N, by, bx, 8, 8])."""
    N, Cc, H, W = x.shape
    T = tables.double()
    p = (x + 1) * 127.5
    if Cc == 3:
        planes = list(torch.einsum('ij,njhw->nihw', COLOUR, p).unbind(1))
        planes[1], planes[2] = planes[1] + 128, planes[2] + 128
    else:
        planes = [p[:, 0]]
    m = mcu_of(Cc, sub)
    Hp, Wp = -(-H // m) * m, -(-W // m) * m
    planes = [F.pad(q[:, None], (0, Wp - W, 0, Hp - H), mode='replicate')[:, 0] for q in planes]
    s420 = m == 16
    if s420:
        planes[1:] = [F.avg_pool2d(q[:, None], 2)[:, 0] for q in planes[1:]]
    out, us = [], []
    for i, q in enumerate(planes):
        t = T[:, min(i, 1), None, None]
        c = DCT @ (_blocks(q) - 128) @ DCT.T
        u = c / t
        r = torch.round(u).detach()
        soft = u if grad == 'ste' else (u - r) ** 3
        chat = (r + (soft - soft.detach())) * t
        out.append(_unblocks(DCT.T @ chat @ DCT) + 128)
        us.append(u)
    if s420:
        out[1:] = [q.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2) for q in out[1:]]
    if Cc == 3:
        ycc = torch.stack([out[0], out[1] - 128, out[2] - 128], dim=1)
        rgb = torch.einsum('ij,njhw->nihw', COLOUR_INV, ycc)
    else:
        rgb = out[0][:, None]
    if clamp:
        rgb = rgb.clamp(0, 255)
    y = rgb[:, :, :H, :W] / 127.5 - 1
    return (y, us) if detail else y


def tables_for(qualities):
    J = pkg('jpeg')
    return torch.from_numpy(np.stack([np.stack(J.quant_tables(int(q))) for q in qualities])).double()


# ---- tables ----------------------------------------------------------------------------------------------------------------------
def test_quant_tables_are_libjpegs():
    J, g = pkg('jpeg'), golden()
    assert g['tables'][list(g['qualities']).index(50), 0, 0].tolist() == [16, 11, 10, 16, 24, 40, 51, 61]      # row-major, Annex K
    for q, t in zip(g['qualities'], g['tables']):
        luma, chroma = J.quant_tables(int(q))
        assert luma.shape == (8, 8) and np.array_equal(luma, t[0]) and np.array_equal(chroma, t[1]), int(q)
    for bad in (0, 101, -3):
        with pytest.raises(ValueError):
            J.quant_tables(bad)


def _host_tables(t, seed, rank, B, qlo, qhi):
    q, tab = np.zeros(B, np.int32), np.zeros((B, 2, 8, 8), np.float32)
    st = pkg('_lib').lib().sisr_jpeg_tables_host(t, seed, rank, B, qlo, qhi, q.ctypes.data_as(C.c_void_p), tab.ctypes.data_as(C.c_void_p))
    assert st == 0
    return q, tab


def _quality_from_philox(seed, t, B, qlo, qhi, rank):
    """rebuilt here from the documented counter, the uniform in float64 (exact: 25 bits), the product rounded to fp32 as the kernel's"""
    r = pkg('draws').draw_words(seed, t, np.arange(B), TAG_QUALITY | rank)
    u0 = (((r[:, 0] >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24).astype(np.float32)
    return np.minimum(qlo + np.floor(np.float32(qhi - qlo + 1) * u0).astype(np.int64), qhi)


@pytest.mark.parametrize('seed,t,rank,qlo,qhi', [(0, 0, 0, 30, 95), ((0xDEADBEEF << 32) | 0x1234567, (5 << 32) + 77, 65535, 1, 100),
                                                 (3, 9, 2, 50, 51)])
def test_quality_draw_host_matches_the_philox_counter(seed, t, rank, qlo, qhi):
    J = pkg('jpeg')
    B = 4096
    q, tab = _host_tables(t, seed, rank, B, qlo, qhi)
    assert np.array_equal(q, J.expected_quality(seed, t, B, qlo, qhi, rank))
    assert np.array_equal(q, _quality_from_philox(seed, t, B, qlo, qhi, rank))
    assert q.min() == qlo and q.max() == qhi                       # both ends are reached over 4096 samples
    for b in (0, 1, B - 1):
        assert np.array_equal(tab[b], np.stack(J.quant_tables(int(q[b]))).astype(np.float32))
    assert not np.array_equal(q, _host_tables(t + 1, seed, rank, B, qlo, qhi)[0])
    assert not np.array_equal(q, _host_tables(t, seed, (rank + 1) % 65536, B, qlo, qhi)[0])


def test_equal_bounds_give_one_quality():
    q, tab = _host_tables(4, 11, 0, 64, 73, 73)
    assert (q == 73).all() and (tab == tab[0]).all()


# ---- the restatement is JPEG -------------------------------------------------------------------------------------------------------
# mean |restatement - Pillow's decoded image| in levels of 255 at 4:4:4 on the committed fixture, measured with the restatement
# above: 1.359 (q = 10), 1.711 (q = 50), 2.149 (q = 90) -- the codec's integer DCT, its 8-bit YCbCr samples on both sides and the
# 8-bit result (the restatement's output is not rounded); the bound is 1.25 x that.  The maximum is not pinned: it reaches a whole quantisation step
# wherever the integer and the float transform round a coefficient differently.
PILLOW_MEAN_ABS = {10: 1.359, 50: 1.711, 90: 2.149}


@pytest.mark.parametrize('q', [10, 50, 90])
def test_restatement_against_pillow_444(q):
    g = golden()
    img = torch.from_numpy(g['image'].astype(np.float64))[None]
    y = jpeg64(img / 127.5 - 1, tables_for([q]), '444', clamp=True)
    ours = (y[0] + 1) * 127.5
    ref = g['roundtrip'][list(g['roundtrip_q']).index(q)].astype(np.float64)
    diff = (ours.numpy() - ref)
    mean, mx = float(np.abs(diff).mean()), float(np.abs(diff).max())
    print('q %d: mean |restatement - Pillow| %.3f levels (bound %.3f), max %.1f' % (q, mean, 1.25 * PILLOW_MEAN_ABS[q], mx))
    assert mean <= 1.25 * PILLOW_MEAN_ABS[q]


def test_restatement_surrogates_and_adjoint():
    """the restatement's own backward: 'ste' at 4:4:4 without clamp on block multiples is the identity; 'cubic' scales by 3 d^2 < 3/4"""
    x = (2 * torch.rand(1, 3, 16, 24, dtype=torch.float64, generator=torch.Generator().manual_seed(0)) - 1).requires_grad_(True)
    dy = torch.randn(1, 3, 16, 24, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    jpeg64(x, tables_for([75]), '444', clamp=False, grad='ste').backward(dy)
    assert float((x.grad - dy).abs().max()) <= 1e-8        # (the colour matrix's nine-digit constants and their float64 inverse)
    gs = x.grad.clone()
    x.grad = None
    jpeg64(x, tables_for([75]), '444', clamp=False, grad='cubic').backward(dy)
    assert 0 < float(x.grad.norm()) < 0.75 * float(gs.norm())


# ---- bad arguments ---------------------------------------------------------------------------------------------------------------
def test_every_bad_argument_is_refused_without_a_gpu():
    lib = pkg('_lib').lib()
    buf = (C.c_float * 4096)()
    p = C.cast(buf, C.c_void_p)           # a non-null pointer: refused calls never read it, and nothing here reaches a launch
    good_tab = dict(step=p, seed=1, rank=0, B=2, qlo=30, qhi=95, q=p, tables=p, stream=None)
    bad_tabs = [dict(step=None), dict(q=None), dict(tables=None), dict(B=0), dict(B=-1), dict(qlo=0), dict(qlo=-5), dict(qhi=101),
                dict(qlo=96), dict(qlo=60, qhi=50), dict(rank=-1), dict(rank=65536)]
    for bad in bad_tabs:
        a = dict(good_tab, **bad)
        assert lib.sisr_jpeg_tables(*a.values()) == BADARG, bad
    good_host = dict(t=0, seed=1, rank=0, B=2, qlo=30, qhi=95, q=p, tables=p)
    assert lib.sisr_jpeg_tables_host(*good_host.values()) == 0
    for bad in [b for b in bad_tabs if 'step' not in b] + [dict(t=-1)]:
        a = dict(good_host, **bad)
        assert lib.sisr_jpeg_tables_host(*a.values()) == BADARG, bad
    good_fwd = dict(x=p, tables=p, y=p, N=1, C=3, H=8, W=8, sub=1, clamp=1, stream=None)
    shapes = [dict(N=0), dict(C=0), dict(C=2), dict(C=4), dict(H=0), dict(W=0), dict(H=-8), dict(sub=2), dict(sub=-1)]
    for bad in [dict(x=None), dict(tables=None), dict(y=None)] + shapes:
        a = dict(good_fwd, **bad)
        assert lib.sisr_jpeg_fwd(*a.values()) == BADARG, bad
    assert lib.sisr_jpeg_fwd(*dict(good_fwd, N=65536).values()) == TOOBIG                 # grid.z
    assert lib.sisr_jpeg_fwd(*dict(good_fwd, H=16 * 65535 + 1).values()) == TOOBIG        # grid.y
    good_bwd = dict(dy=p, y=None, x=None, tables=None, dx=p, N=1, C=3, H=8, W=8, sub=1, grad=0, stream=None)
    for bad in [dict(dy=None), dict(dx=None), dict(grad=2), dict(grad=-1), dict(grad=1), dict(grad=1, x=p), dict(grad=1, tables=p)] + shapes:
        a = dict(good_bwd, **bad)
        assert lib.sisr_jpeg_bwd(*a.values()) == BADARG, bad
    assert lib.sisr_jpeg_bwd(*dict(good_bwd, N=65536).values()) == TOOBIG
    assert lib.sisr_jpeg_bwd(*dict(good_bwd, H=16 * 65535 + 1).values()) == TOOBIG


def test_python_surface_refuses_what_the_library_would():
    J, D = pkg('jpeg'), pkg('degrade')
    with pytest.raises(RuntimeError):
        J.jpeg_roundtrip(torch.zeros(1, 3, 8, 8), 75)                  # a CPU tensor: no fallback
    for bad in (dict(qlo=0, qhi=5), dict(qlo=9, qhi=8), dict(qlo=1, qhi=101), dict(B=0), dict(t=-1), dict(rank=65536), dict(seed=-1)):
        with pytest.raises(ValueError):
            J.expected_quality(**dict(dict(seed=0, t=0, B=4, qlo=30, qhi=95, rank=0), **bad))
    with pytest.raises(RuntimeError):
        D.Degrader(device='cpu', jpeg=(30, 95))
