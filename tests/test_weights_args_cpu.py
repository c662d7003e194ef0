"""CPU: argument rejection of the weight-side entry points (csrc/spectral.hip), the closed form of sisr_weights_grad_tiles, and the
conditions on the seeded inputs of tests/test_gpu_weights.py that need no device.

Every rejection below is read off the wrapper's source: the argument set fails a check that sits BEFORE the first
hipLaunchKernelGGL, so the call returns SISR_E_BADARG without touching a device and the pointers (made-up addresses) are never
dereferenced.  tests/test_gpu_weights.py holds the value tests of the same entry points."""
import ctypes as C
import importlib

import pytest

import weights_cases as WC

BADARG = -1                             # include/sisr_hip.h
P = 0x10000                             # a made-up, 16-byte aligned, non-null device address
NUL = None


@pytest.fixture(scope='module')
def L():
    return importlib.import_module('single-image-super-resolution_amd._lib')


def _cases():
    c = []

    def add(fn, what, *args):
        c.append(pytest.param(fn, args, id='%s-%s' % (fn[5:], what)))

    # sisr_weights_sn / _pack / _prepare(table, n, max_rows, max_cols, stream); _pack_deep(table, n, max_cout, max_cin, stream)
    ok = [P, 3, 64, 576, NUL]
    for fn in ('sisr_weights_sn', 'sisr_weights_pack', 'sisr_weights_prepare', 'sisr_weights_pack_deep'):
        for what, i, v in (('null_table', 0, NUL), ('n0', 1, 0), ('n_neg', 1, -2), ('rows0', 2, 0), ('rows_neg', 2, -64),
                           ('cols0', 3, 0), ('cols_neg', 3, -576)):
            add(fn, what, *(ok[:i] + [v] + ok[i + 1:]))
    # sisr_weights_grad(table, n, dot_work, parts, stream)
    ok = [P, 3, P, 36, NUL]
    for what, i, v in (('null_table', 0, NUL), ('n0', 1, 0), ('n_neg', 1, -1), ('null_dot_work', 2, NUL), ('parts0', 3, 0),
                       ('parts_neg', 3, -36), ('parts_65536', 3, 65536)):
        add('sisr_weights_grad', what, *(ok[:i] + [v] + ok[i + 1:]))
    # sisr_weights_grad_fast(table, n, dot_work, max_cout, max_cin, stream)
    ok = [P, 3, P, 64, 64, NUL]
    for what, i, v in (('null_table', 0, NUL), ('n0', 1, 0), ('n_neg', 1, -1), ('null_dot_work', 2, NUL), ('cout0', 3, 0),
                       ('cout_neg', 3, -64), ('cin31', 4, 31), ('cin0', 4, 0), ('cin_neg', 4, -32)):
        add('sisr_weights_grad_fast', what, *(ok[:i] + [v] + ok[i + 1:]))
    return c


@pytest.mark.parametrize('fn,args', _cases())
def test_weights_entry_point_rejects_before_launch(L, fn, args):
    assert getattr(L.lib(), fn)(*args) == BADARG


def _tiles(L, cout, cin, kh, kw, ck, layout):
    t = L.WeightGradDesc()
    t.Cout, t.Cin, t.KH, t.KW, t.CK, t.layout = cout, cin, kh, kw, ck, layout
    return L.lib().sisr_weights_grad_tiles(C.byref(t))


@pytest.mark.parametrize('shape,layout,seed', WC.all_grad_cases())
def test_weights_grad_tiles_closed_form(L, shape, layout, seed):
    """tiles = ceil(Cout / 32) * ceil(Cin / C) * ceil(taps / tg), tg = clamp(32 / min(C, Cin), 1, taps); C = 32 for layout 1, the
    plan's CK otherwise (include/sisr_hip.h)"""
    cout, cin, k, _ = shape
    ck = WC.wgrad_plan(cout, cin, k, layout)['CK']
    want, tg = WC.tiles_closed_form(cout, cin, k, 32 if layout == 1 else ck)
    # layout 1 ignores CK
    assert _tiles(L, cout, cin, k, k, 0 if layout == 1 else ck, layout) == want
    # worked by hand: the branches the value tests rely on
    by_hand = {((64, 64, 3, 0), 0): (2 * 2 * 9, 1), ((48, 40, 3, 0), 0): (2 * 2 * 9, 1), ((64, 3, 9, 0), 0): (2 * 1 * 9, 10),
               ((40, 24, 3, 1), 0): (2 * 1 * 9, 1), ((3, 64, 3, 0), 0): (1 * 2 * 9, 1), ((16, 1, 3, 0), 0): (1 * 1 * 1, 9),
               ((64, 64, 1, 0), 0): (2 * 2 * 1, 1), ((256, 64, 3, 1), 1): (8 * 2 * 9, 1), ((4, 64, 3, 0), 1): (1 * 2 * 9, 1)}
    if (shape, layout) in by_hand:
        assert (want, tg) == by_hand[(shape, layout)]


@pytest.mark.parametrize('field', ['Cout', 'Cin', 'KH', 'KW'])
def test_weights_grad_tiles_rejects_zero_dimensions(L, field):
    dims = {'Cout': 64, 'Cin': 64, 'KH': 3, 'KW': 3}
    for bad in (0, -1):
        d = dict(dims, **{field: bad})
        for layout, ck in ((0, 32), (1, 32)):
            assert _tiles(L, d['Cout'], d['Cin'], d['KH'], d['KW'], ck, layout) == BADARG


def test_weights_grad_tiles_rejects_missing_chunk_size(L):
    assert L.lib().sisr_weights_grad_tiles(None) == BADARG
    for ck in (0, -32):
        assert _tiles(L, 64, 64, 3, 3, ck, 0) == BADARG
        assert _tiles(L, 64, 64, 3, 3, ck, 1) == 2 * 2 * 9            # layout 1 has fixed chunks of 32


@pytest.mark.parametrize('shape,layout,seed', WC.all_grad_cases())
def test_epilogue_inputs_meet_their_conditions(shape, layout, seed):
    """rho = |(<G, W_orig> / sigma) u v^T|_F / |G|_F >= 0.25 and NaN in every padding slot of the slab, for every seeded case"""
    c = WC.grad_case(shape, layout, seed)
    c.check_inputs()
    print('%s layout %d: rho %.3f, %d padding slots of %d' % (shape, layout, c.rho, c.n_pad, c.slab.numel()))
    if (shape, layout) == ((48, 40, 3, 0), 0):
        assert c.plan['CK'] == 32 and c.plan['n_chunk'] == 2          # second chunk ragged: 8 channels
    if (shape, layout) == ((64, 3, 9, 0), 0):
        assert c.tg == 10 and 81 % 10 == 1                            # nine tap groups, the last holds one tap


# ---- packed weight images: what tests/test_gpu_weight_images.py needs without a device ---------------------------------------------
@pytest.fixture(scope='module')
def E():
    return importlib.import_module('single-image-super-resolution_amd.engine')


@pytest.mark.parametrize('build', ['fp32', 'bf16x3', 'bf16'])
def test_image_references_have_the_images_sizes_and_count_every_padding_slot(E, build):
    """every layer of the image table reaches the format it is listed for; each reference image is as long as the engine's size
    formulas say (plan.wpk_elems + the LDS-order words, ceil(wpk_elems / 2) twice with the lane-order copy, ceil(wimg_elems / 2), the
    KW = 2 rows of the one-launch stride-2 plan), and its standard order holds exactly one element per (cout, cin, forward tap the
    image reaches) -- every other slot is a zero the comparison counts"""
    import torch
    n_images = 0
    for i, (gm, _, p) in enumerate(WC.image_layers(E, build)):
        WC.check_reach(E, build, i, p)
        wm = WC.sn_inputs((gm.cout, gm.cin, gm.k), seed=60 + i)[0]
        w4 = wm.reshape(gm.cout, gm.cin, gm.k, gm.k)
        assert bool((w4.to(torch.bfloat16) != 0).all())
        for spec in WC.image_specs(E, p):
            if spec is None:
                continue
            slots, std = WC.expected_image(spec, w4, torch.tensor(0.75), gm.shuffle2)
            assert slots.numel() == spec.old_slots, (build, i, spec.name, slots.numel(), spec.old_slots)
            kh, kw, r0y, sy, r0x, sx = spec.taps
            reached = sum(0 <= r0y + sy * a < gm.k for a in range(kh)) * sum(0 <= r0x + sx * b < gm.k for b in range(kw))
            assert int((std != 0).sum()) == gm.cout * gm.cin * reached, (build, i, spec.name)
            n_images += 1
    assert n_images == {'fp32': 15, 'bf16x3': 2, 'bf16': 23}[build]


def _plan_digest_layers():
    """the layer list of tools/plan_digest.py (imported from the module the tool imports it from: the lists cannot drift apart)"""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location(
        'plan_layers', os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools', 'plan_layers.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return list(mod.LAYERS)


@pytest.mark.parametrize('build', ['fp32', 'bf16x3', 'bf16'])
def test_library_image_sizes_equal_the_engines_former_formulas(E, L, build):
    """sisr_weight_image_bytes, the one place that knows an image's size, against the formulas the engine used to carry (they live
    on in weights_cases.image_specs): every image of the fourteen layers of the image table and of tools/plan_digest.py's layer
    list, and the layout's (offset, length) records, which must tile the buffers in 16-byte steps"""
    layers = [(cin, cout, k, s, bool(sh), False, 2, h, w) for cin, cout, k, s, sh, h, w in WC.IMAGE_CASES[build]] + _plan_digest_layers()
    assert len(layers) == len(WC.IMAGE_CASES[build]) + 17
    before = E.PRECISION
    E.set_precision(build)
    try:
        items = [(E.ConvRef(E.ConvGeom(cin, cout, k, s, shuffle2=sh, deep_dgrad=dd), None, None), n, h, w)
                 for cin, cout, k, s, sh, dd, n, h, w in layers]
        preps, offs, sizes = E._layout_weights(items, True)
        used, n_images = {'b': 0, 'd': 0}, 0
        for p, (imgs, _, _) in zip(preps, offs):
            specs = WC.image_specs(E, p)
            assert [s is None for s in specs] == [i is None for i in imgs]
            for spec, img in zip(specs, imgs):
                if spec is None:
                    continue
                assert L.lib().sisr_weight_image_bytes(C.byref(img.rec)) == 4 * spec.old_slots, (build, spec.name)
                assert img.slots == spec.old_slots and img.buf == ('d' if spec.fmt == WC.IMG_DEEP else 'b')
                assert img.off == used[img.buf] and img.off % 4 == 0
                used[img.buf] += (img.slots + 3) & ~3
                n_images += 1
        assert (used['b'], used['d']) == (sizes['b'], sizes['d']) and n_images >= 2 * len(layers)
    finally:
        E.set_precision(before)


def test_weight_image_bytes_rejects_records_no_kernel_packs(L):
    def rec(**kw):
        g = L.WeightImage()
        g.format, g.KH, g.KW, g.CK, g.PS, g.KROWP, g.n_chunk, g.CoutPad = L.WIMG_F32, 3, 3, 32, 33, 100, 2, 64
        for n, v in kw.items():
            setattr(g, n, v)
        return g
    lib = L.lib()
    assert lib.sisr_weight_image_bytes(None) == BADARG
    assert lib.sisr_weight_image_bytes(C.byref(rec())) == 4 * 2 * 3 * 64 * 100          # dst is not read
    assert lib.sisr_weight_image_bytes(C.byref(rec(extra=2))) == 4 * (2 * 3 * 64 * 100 + 2 * 2 * 9 * 32 * 36)
    assert lib.sisr_weight_image_bytes(C.byref(rec(format=L.WIMG_BF16, extra=1))) == 2 * 2 * (2 * 64 * 9 * 32)
    assert lib.sisr_weight_image_bytes(C.byref(rec(format=L.WIMG_DEEP, KH=2, KW=1, extra=2))) == 2 * (2 * 2 * 64 * 72)
    for bad in (dict(format=3), dict(format=-1), dict(KH=0), dict(KW=-3), dict(n_chunk=0), dict(CoutPad=0), dict(KROWP=0), dict(PS=0),
                dict(CK=0), dict(extra=3), dict(extra=-1), dict(format=L.WIMG_BF16, extra=2), dict(format=L.WIMG_BF16, CK=0),
                dict(format=L.WIMG_DEEP, extra=2), dict(format=L.WIMG_DEEP, extra=0)):
        assert lib.sisr_weight_image_bytes(C.byref(rec(**bad))) == BADARG, bad
