"""CPU: sisr_toimage_bwd_f32_eligible (pure host code) accepts the generator's last conv at the geometry toimage_bwd.hip is
written for -- 3x3, 64 -> 3, stride 1, pad 1, H % 8 == 0, W % 32 == 0, fp32 tensors, tensor bytes < 2^31 -- and rejects each
single deviation; SISR_TOIMAGE_BWD=0 / SISR_THIN=0 keep the separate kernels; the Python mirror of the descriptor has the
library's size."""
import ctypes as C
import importlib

import pytest

PKG = 'single-image-super-resolution_amd'
SWITCHES = ('SISR_TOIMAGE_BWD', 'SISR_THIN', 'SISR_PERSIST_MAX_WG')


def _pkg(sub):
    return importlib.import_module(PKG + '.' + sub)


def _desc(n=16, h=192, w=192):
    """the descriptor engine.toimage_backward builds for the bench's end conv, from the planners alone (no tensors)"""
    E, L = _pkg('engine'), _pkg('_lib')
    E.set_precision('fp32')
    f, _, g, kinds = E.ConvGeom(64, 3, 3, 1, 1).plans(n, h, w)
    assert kinds == (False, False, False)
    d = L.ToImageBwdDesc()
    for name in ('N', 'H', 'W', 'Cin', 'Cout', 'KH', 'KW', 'stride', 'pad_y', 'pad_x', 'CK', 'PS', 'KROWP', 'n_chunk', 'CoutPad',
                 'slab_elems', 'slab_stride'):
        setattr(d, name, getattr(g, name))
    d.w_CK, d.w_PS, d.w_KROWP, d.w_CoutPad = f.plan.CK, f.plan.PS, f.plan.KROWP, f.plan.CoutPad
    return d


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for v in SWITCHES:
        monkeypatch.delenv(v, raising=False)


def test_descriptor_mirror_has_the_library_size():
    L = _pkg('_lib')
    assert L.lib().sisr_toimage_bwd_desc_bytes() == C.sizeof(L.ToImageBwdDesc)


@pytest.mark.parametrize('shape', [(16, 192, 192), (2, 8, 32), (3, 24, 64), (1, 96, 96)])
def test_the_geometry_is_accepted(shape):
    lib = _pkg('_lib').lib()
    d = _desc(*shape)
    assert lib.sisr_toimage_bwd_f32_eligible(C.byref(d)) == 1
    tiles = shape[0] * (shape[1] // 8) * (shape[2] // 32)
    assert 1 <= lib.sisr_toimage_bwd_f32_parts(C.byref(d)) <= tiles           # one slab per workgroup, no workgroup without a tile


@pytest.mark.parametrize('field,value', [
    ('H', 188), ('H', 13),                  # H % 8
    ('W', 176), ('W', 31),                  # W % 32
    ('Cin', 32), ('Cin', 128),
    ('Cout', 4), ('Cout', 1),
    ('KH', 1), ('KW', 5),                   # kernel size
    ('stride', 2),
    ('pad_y', 0), ('pad_x', 2),
    ('pre_bf16', 1), ('g_bf16', 1),         # bf16 tensors
    ('N', 228),                             # 228 x 192 x 192 x 256 bytes >= 2^31 (227 is the last that fits)
])
def test_each_single_deviation_is_rejected(field, value):
    lib = _pkg('_lib').lib()
    d = _desc()
    assert lib.sisr_toimage_bwd_f32_eligible(C.byref(d)) == 1
    setattr(d, field, value)
    assert lib.sisr_toimage_bwd_f32_eligible(C.byref(d)) == 0, (field, value)
    assert lib.sisr_toimage_bwd_f32(C.byref(d), None) != 0                      # ... and the launch refuses it (before any HIP call)


def test_the_byte_limit_is_exact():
    lib = _pkg('_lib').lib()
    d = _desc()
    d.N = 227                                                                   # 227 * 192 * 192 * 256 = 2^31 - 5,210,112
    assert d.N * d.H * d.W * 256 < 2 ** 31 and lib.sisr_toimage_bwd_f32_eligible(C.byref(d)) == 1
    d.N, d.H, d.W = 1, 2048, 4096                                               # exactly 2^31 bytes
    assert d.N * d.H * d.W * 256 == 2 ** 31 and lib.sisr_toimage_bwd_f32_eligible(C.byref(d)) == 0


@pytest.mark.parametrize('switch', ['SISR_TOIMAGE_BWD', 'SISR_THIN'])
def test_switches_keep_the_separate_kernels(monkeypatch, switch):
    lib = _pkg('_lib').lib()
    d = _desc()
    monkeypatch.setenv(switch, '0')
    assert lib.sisr_toimage_bwd_f32_eligible(C.byref(d)) == 0
    monkeypatch.setenv(switch, '1')
    assert lib.sisr_toimage_bwd_f32_eligible(C.byref(d)) == 1


def test_null_descriptor_and_unbound_tensors_are_refused():
    lib = _pkg('_lib').lib()
    assert lib.sisr_toimage_bwd_f32_eligible(None) == 0
    d = _desc()
    assert lib.sisr_toimage_bwd_f32(C.byref(d), None) == -1                     # SISR_E_BADARG: no tensor bound
