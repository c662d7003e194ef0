"""CPU: the host side of whole-image super-resolution (upscale.py, csrc/tiles.hip) -- the axis planner
(sisr_tile_axis: host code of the library), receptive_halo, the numpy restatement of the stitch weights, the argument checks of
sisr_tile_gather_f32 / sisr_tile_stitch (refused before any HIP call) and the command-line tool's argument handling."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from helpers import load_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = 'single-image-super-resolution_amd'
BADARG = -1


def _pkg(sub):
    return importlib.import_module(PKG + '.' + sub)


def _tool():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        return importlib.import_module('upscale_image')
    finally:
        sys.path.pop(0)


# ---- planner ---------------------------------------------------------------------------------------------------------------------
CASES = [(L, T, halo) for T in (8, 16, 33) for halo in (0, 1, 3) for L in range(1, 81)]


def test_planner_properties():
    U = _pkg('upscale')
    lib = _pkg('_lib').lib()
    for L, T, halo in CASES:                                         # core = T - 2 halo >= 2 in all of them
        a, b = (v.astype(np.int64) for v in U.tile_axis(L, T, halo))
        n, t = len(a), min(T, L)
        what = (L, T, halo, a.tolist(), b.tolist())
        if L <= T:
            assert n == 1 and a[0] == 0 and b[0] == L, what
        else:
            assert n == -(-(L - 2 * halo) // (T - 2 * halo)) and n >= 2, what
            assert np.array_equal(a, np.minimum(np.arange(n) * (T - 2 * halo), L - T)), what
        assert n == lib.sisr_tile_axis(L, T, halo, None, None, 0), what
        lo = np.concatenate([[0], b[:-1]])                           # tile i owns [lo_i, b_i)
        assert b[-1] == L and (b > lo).all(), what                   # the owned intervals partition [0, L), none empty
        assert (a >= 0).all() and (a + t <= L).all(), what           # every window inside the image
        assert a[0] == 0 and a[-1] + t == L, what                    # border windows flush with the border
        assert (np.diff(a) > 0).all(), what                          # origins strictly increasing
        for i in range(n):                                           # owned pixels >= halo from each interior window edge
            assert lo[i] >= a[i] and b[i] <= a[i] + t, what
            if a[i] > 0:
                assert lo[i] - a[i] >= halo, what
            if a[i] + t < L:
                assert a[i] + t - b[i] >= halo, what
    for L, T, halo in ((9, 8, 4), (80, 6, 3), (100, 33, 17)):        # core < 1: refused
        assert lib.sisr_tile_axis(L, T, halo, None, None, 0) == BADARG
        with pytest.raises(ValueError):
            U.tile_axis(L, T, halo)
    assert lib.sisr_tile_axis(8, 8, 4, None, None, 0) == 1           # L <= T: one tile, whatever the halo


def test_planner_argument_checks():
    lib = _pkg('_lib').lib()
    a, b = np.zeros(8, np.int32), np.zeros(8, np.int32)
    pa, pb = a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p)
    assert lib.sisr_tile_axis(40, 16, 3, pa, pb, 8) == 4
    assert lib.sisr_tile_axis(0, 16, 3, pa, pb, 8) == BADARG
    assert lib.sisr_tile_axis(40, 0, 0, pa, pb, 8) == BADARG
    assert lib.sisr_tile_axis(40, 16, -1, pa, pb, 8) == BADARG
    assert lib.sisr_tile_axis(40, 16, 3, pa, None, 8) == BADARG
    assert lib.sisr_tile_axis(40, 16, 3, pa, pb, 0) == BADARG
    assert lib.sisr_tile_axis(40, 16, 3, pa, pb, 3) == -2            # SISR_E_TOOBIG: four tiles, room for three


def test_tile_plan_is_the_row_major_outer_product():
    U = _pkg('upscale')
    p = U.TilePlan(45, 61, 16, 3)
    assert (p.ny, p.nx, p.n, p.th, p.tw) == (4, 6, 24, 16, 16)
    assert p.table.shape == (24, 4) and p.table.dtype == np.int32
    for t in range(p.n):
        assert p.table[t].tolist() == [0, p.ay[t // p.nx], p.ax[t % p.nx], 0]
    e = p.ensemble_table(8)
    assert e.shape == (192, 4) and np.array_equal(e[:, 3], np.repeat(np.arange(8), 24)) and np.array_equal(e[48:72, :3], p.table[:, :3])
    q = U.TilePlan(11, 61, 16, 3)                                    # smaller than the tile on one axis
    assert (q.ny, q.nx, q.th, q.tw) == (1, 6, 11, 16)


# ---- receptive field -------------------------------------------------------------------------------------------------------------
def test_receptive_halo():
    U, mg, mp = _pkg('upscale'), _pkg('model_generator'), _pkg('model_generator_progressive')
    for scales in ([2], [2, 2], [2, 2, 2]):
        assert U.receptive_halo(mg.Generator(16, 64, 256, scales)) == 40, scales
    small = mg.Generator(2, 16, 64, [2])
    assert U.receptive_halo(small) == 12
    assert U.receptive_halo(mg.GeneratorSuffix(small)) == 12         # 4 -> 3 -> 3, + 1 + 4 + 4
    base = mp.GeneratorProgresiveBase(3, 16)                         # no end conv, no stage: 0 + 1 + 2 * 3 + 4
    assert U.receptive_halo(base) == 11
    g1 = mp.GeneratorSuffix(base, 16)
    assert U.receptive_halo(g1.beginning) == 12                      # no end conv, one stage: ceil(0 / 2) + 1 = 1, + 11
    assert U.receptive_halo(g1) == 14                                # end conv: 4 -> 3, + 11
    assert U.receptive_halo(mp.GeneratorSuffix(g1.beginning, 4)) == 14      # 4 -> 3 -> 3


# ---- weight formula --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('s', [2, 4])
def test_axis_weights_sum_to_one_inside_their_windows(s):
    U = _pkg('upscale')
    for L, T, halo in ((45, 16, 3), (61, 16, 3), (11, 16, 3), (80, 8, 3), (80, 33, 1), (50, 16, 0), (17, 16, 3)):
        a, b = U.tile_axis(L, T, halo)
        t = min(T, L)
        for f in sorted({0, 1, halo} & set(range(halo + 1))):
            w = U.axis_weights(b, s, f, L)
            assert w.shape == (len(a), s * L) and np.isfinite(w).all() and (w >= 0).all(), (L, T, halo, f)
            assert np.abs(w.sum(axis=0) - 1.0).max() < 1e-12, (L, T, halo, f)
            Y = np.arange(s * L)
            inside = (Y[None, :] >= s * a[:, None]) & (Y[None, :] < s * (a[:, None] + t))
            assert not (w[~inside] > 0).any(), (L, T, halo, f)       # a weight's support lies inside its tile's window
            owner = np.searchsorted(b, (Y + 0.5) / s, side='right')
            assert (w[owner, Y] > 0).all(), (L, T, halo, f)         # the owner always carries weight (raw: at least 1/2)
            if f == 0:
                assert np.array_equal(w, (np.arange(len(a))[:, None] == owner[None, :]).astype(np.float64)), (L, T, halo)


# ---- argument refusal: SISR_E_BADARG before any HIP call (no GPU here: a launch would fail with another status) ------------------
STITCH_OK = dict(tiles=64, table=64, ay=64, by=64, ny=4, ax=64, bx=64, nx=6, C=3, H=45, W=61, th=16, tw=16, scale=2, halo=3,
                 feather=1.0, E=1, mean=0.5, stdv=0.5, dst=64, dst_kind=0)
STITCH_BAD = ([(k, None) for k in ('tiles', 'table', 'ay', 'by', 'ax', 'bx', 'dst')] +
              [(k, 0) for k in ('ny', 'nx', 'C', 'H', 'W', 'th', 'tw', 'scale')] +
              [('scale', 3), ('scale', 16), ('scale', -2), ('E', 0), ('E', 2), ('E', 4), ('E', 9), ('C', 5), ('th', 46), ('tw', 62),
               ('feather', -0.5), ('feather', 3.5), ('feather', float('nan')), ('halo', -1), ('dst_kind', 2)])


def _stitch(lib, **over):
    a = dict(STITCH_OK, **over)
    return lib.sisr_tile_stitch(*[a[k] for k in STITCH_OK], None)


@pytest.mark.parametrize('field,value', STITCH_BAD)
def test_stitch_refuses_each_bad_argument(field, value):
    assert _stitch(_pkg('_lib').lib(), **{field: value}) == BADARG, (field, value)


def test_stitch_refuses_an_ensemble_over_oblong_tiles():
    lib = _pkg('_lib').lib()
    assert _stitch(lib, E=8, th=16, tw=24) == BADARG and _stitch(lib, E=8, th=11, tw=16, H=11) == BADARG


GATHER_OK = dict(src=64, C=3, H=45, W=61, table=64, n=24, th=16, tw=16, dst=64)


@pytest.mark.parametrize('field,value', [('src', None), ('table', None), ('dst', None), ('C', 0), ('C', 5), ('H', 0), ('W', 0),
                                         ('n', 0), ('th', 0), ('tw', 0), ('th', 46), ('tw', 62)])
def test_gather_refuses_each_bad_argument(field, value):
    a = dict(GATHER_OK, **{field: value})
    assert _pkg('_lib').lib().sisr_tile_gather_f32(*[a[k] for k in GATHER_OK], None) == BADARG, (field, value)


# ---- the public interface without a GPU ------------------------------------------------------------------------------------------
def test_upscaler_refuses_cpu_tensors_and_other_inputs():
    U, mg = _pkg('upscale'), _pkg('model_generator')
    up = U.Upscaler(mg.Generator(2, 16, 64, [2]), tile=32)
    assert (up.halo, up.scale) == (12, 2)
    for image in (torch.zeros(20, 27, 3, dtype=torch.uint8), torch.zeros(3, 20, 27)):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            up(image)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        up.to_float(torch.zeros(20, 27, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        U.evaluate_image(up, torch.zeros(40, 54, 3, dtype=torch.uint8))
    for image in (torch.zeros(1, 3, 20, 27), torch.zeros(20, 27, 3, dtype=torch.int32), torch.zeros(3, 20, 27, dtype=torch.float64),
                  np.zeros((20, 27, 3), np.uint8), torch.zeros(20, 27, 5, dtype=torch.uint8)):
        with pytest.raises(RuntimeError):
            up(image)


def test_upscaler_checks_its_settings():
    U, mg = _pkg('upscale'), _pkg('model_generator')
    net = mg.Generator(2, 16, 64, [2])
    for kw in (dict(tile=0), dict(batch=0), dict(halo=-1), dict(ensemble=4), dict(feather=-1), dict(feather=13), dict(halo=2, feather=3),
               dict(std=0.0)):
        with pytest.raises(ValueError):
            U.Upscaler(net, **kw)
    up = U.Upscaler(net, tile=24)                                    # halo 12: no core
    assert up.plan(20, 24).n == 1                                    # ... which an image inside one tile does not need
    with pytest.raises(ValueError, match='tile >= 25'):
        up.plan(45, 61)
    up8 = U.Upscaler(net, tile=32, ensemble=8)
    assert up8.plan(45, 61).n == 15 and up8.plan(20, 20).n == 1
    with pytest.raises(ValueError, match='tile=20 with halo <= 9 would work'):         # halo 12 leaves a 20-pixel tile no core
        up8.plan(20, 61)
    with pytest.raises(ValueError, match='tile=20 would work'):
        U.Upscaler(net, tile=32, ensemble=8, halo=4).plan(20, 61)
    assert U.Upscaler(net, tile=20, ensemble=8, halo=4).plan(20, 61).th == 20


# ---- command-line tool -------------------------------------------------------------------------------------------------------------
def test_cli_arguments():
    T = _tool()
    a = T.parse_args(['ck.pth', 'in.png', 'out.png'])
    assert (a.checkpoint, a.input, a.output, a.tile, a.halo, a.feather, a.ensemble, a.batch, a.ema) == \
        ('ck.pth', 'in.png', 'out.png', 192, None, 0.0, 1, 8, False)
    a = T.parse_args(['ck.pth', 'in.png', 'out.png', '--tile', '96', '--halo', '16', '--feather', '4', '--ensemble', '8', '--ema'])
    assert (a.tile, a.halo, a.feather, a.ensemble, a.ema) == (96, 16, 4.0, 8, True)
    for bad in (['--tile', '0'], ['--halo', '-1'], ['--feather', '-1'], ['--halo', '4', '--feather', '5'], ['--ensemble', '4'],
                ['--batch', '0']):
        with pytest.raises(SystemExit):
            T.parse_args(['ck.pth', 'in.png', 'out.png'] + bad)
    with pytest.raises(SystemExit):
        T.parse_args(['ck.pth', 'in.png'])


@pytest.mark.parametrize('case', ['gen_x2_sn_w64', 'gen_x2_nosn_w16', 'gen_x4_scales22_w32', 'gen_x4_suffix_w32', 'gen_x8_suffix2_w16'])
def test_cli_reads_the_architecture_off_a_reference_state_dict(case, capsys):
    T = _tool()
    _, cfg, state, _, _ = load_case(case)
    arch = T.arch_from_state(state)
    assert arch == dict(n_blocks=cfg['n_blocks'], n_features_block=cfg['nf'], n_features_last=cfg['nl'],
                        list_scales=cfg['list_scales'], use_sn=cfg['use_sn'], input_channels=3, n_suffix=cfg['n_suffix'])
    net = T.build_generator(state)
    assert capsys.readouterr().out == ''                             # full coverage: nothing to report
    sd = net.state_dict()
    assert list(sd.keys()) == list(state.keys()) and all(torch.equal(sd[k], v) for k, v in state.items())
    assert _pkg('upscale').Upscaler(net).scale == 2 ** (len(cfg['list_scales']) + cfg['n_suffix'])
    with pytest.raises(ValueError):
        T.arch_from_state({k: v for k, v in state.items() if 'end.0.' not in k})
