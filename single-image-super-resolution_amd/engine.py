"""Host-side engine: turns the reference's layers into launches of the gfx950 kernels.

PyTorch is plumbing here (device memory through the caching allocator, the current HIP stream,
autograd bookkeeping); every FLOP of the path runs in libsisr_hip.so.  An activation is carried
as a *lazy operand*: a raw NHWC tensor plus the per-channel affine (BatchNorm apply) and the
leaky-relu slope (PReLU / LeakyReLU / ReLU) that its consumer applies while staging tiles into
LDS, so BatchNorm / activation layers never make their own pass over HBM.
"""
import ctypes as C
import enum
import os
from collections import namedtuple

import torch

from . import _lib as L

# 'fp32': exact-fp32 MFMA everywhere (the parity build).  'bf16': layers with Cin % 32 == 0 run their
# contraction on the bf16 matrix cores (fp32 accumulate, fp32 statistics) and keep their NHWC tensors as bf16 in HBM
# (storage_bf16() below).
PRECISION = os.environ.get('SISR_PRECISION', 'fp32')


def _knob(name, default):
    """an environment switch, read when it is used (tests set them between calls)"""
    return os.environ.get(name, default)


def _on(name):
    """an on / off switch: on unless the environment says NAME=0"""
    return os.environ.get(name, '1') != '0'


def set_precision(p):
    """'fp32': fp32 tensors, exact fp32 matrix instructions.  'bf16x3': fp32 tensors and arithmetic as 'fp32', the trunk
    contractions on the bf16 matrix instruction over (hi, lo) bf16 pairs of every fp32 operand (SisrConvDesc.mfma_split; operands
    good to 2^-17 relative -- inside the 1e-3 parity bar by two orders of magnitude).  'bf16': bf16 tensors in HBM."""
    global PRECISION
    assert p in ('fp32', 'bf16x3', 'bf16')
    PRECISION = p


def mfma_split():
    return int(PRECISION == 'bf16x3')


def storage_bf16():
    """bf16 build: NHWC activation / gradient tensors whose channel count is a multiple of 32 live in HBM as bf16
    (SURVEY 8d's bf16 bytes); arithmetic, accumulation and BatchNorm statistics stay fp32.  SISR_STORAGE=f32 keeps
    fp32 tensors with bf16 matrix-core operands (the earlier layout; A/B switch)."""
    return PRECISION == 'bf16' and _knob('SISR_STORAGE', 'bf16') != 'f32'


def act_dtype(channels=64):
    return torch.bfloat16 if storage_bf16() and channels % 32 == 0 else torch.float32


def _bf(t):
    return int(t is not None and t.dtype == torch.bfloat16)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _copy_struct(s):
    return type(s).from_buffer_copy(s)


def _align4(n):
    return (n + 3) & ~3


def _slope(s):
    """a leaky slope (device scalar tensor | float | None = identity) -> (device pointer | None, float) as the descriptors take it"""
    if isinstance(s, torch.Tensor):
        return s.data_ptr(), 1.0
    return None, 1.0 if s is None else float(s)


class Kind(enum.IntEnum):
    """the kernel family one role (forward, data gradient, weight gradient) of a layer is planned for.  (An IntEnum from 0 so that
    tests and tools may go on reading a kind as "runs on a bf16 kernel" by truth value.)"""
    F32 = 0             # the exact-fp32 kernels (fp32 tensors; 'bf16x3' splits their operands)
    BF16 = 1            # the generic bf16 kernels and the persistent trunk kernels behind the same entry point
    DEEP = 2            # conv_deep.hip: split-K implicit GEMM with a weight image of its own
    DEEP_S2X4 = 3       # conv_deep.hip, ONE launch over the four output-parity classes of a stride-2 data gradient

    @property
    def bf16(self):
        """runs on a bf16-tensor kernel (the sisr_conv2d_bf16 / sisr_conv2d_wgrad_bf16 entry points)"""
        return self != Kind.F32

    @property
    def deep(self):
        """the conv_deep.hip family"""
        return self in (Kind.DEEP, Kind.DEEP_S2X4)


# the library's entry points per tensor family, keyed by Kind.bf16: every call site asks this table.  (The two families size the
# BatchNorm-backward rows through different calls; the fp32 kernels' slabs are never bf16, so that family has no slab_lead.)
Family = namedtuple('Family', 'conv parts bnb_parts trunk_eligible wgrad wgrad_route slabs slab_lead batch_arg_bytes batch_args batch')
_FAMILY = {
    False: Family('sisr_conv2d_f32', 'sisr_conv2d_f32_parts', 'sisr_conv2d_f32_bnb_parts', 'sisr_conv2d_trunk_f32_eligible',
                  'sisr_conv2d_wgrad_f32', 'sisr_wgrad_f32_route', 'sisr_wgrad_f32_slabs', None,
                  'sisr_wgrad_trunk_f32_batch_arg_bytes', 'sisr_wgrad_trunk_f32_batch_args', 'sisr_wgrad_trunk_f32_batch'),
    True: Family('sisr_conv2d_bf16', 'sisr_conv2d_bf16_parts', 'sisr_conv2d_bf16_parts', 'sisr_conv2d_trunk_eligible',
                 'sisr_conv2d_wgrad_bf16', 'sisr_wgrad_bf16_route', 'sisr_wgrad_bf16_slabs', 'sisr_wgrad_bf16_slab_lead',
                 'sisr_wgrad_trunk_batch_arg_bytes', 'sisr_wgrad_trunk_batch_args', 'sisr_wgrad_trunk_batch'),
}


def _entry(bf16, what):
    """the library function behind entry point `what` (a field of Family) in the tensor family of a Kind.bf16"""
    return getattr(L.lib(), getattr(_FAMILY[bool(bf16)], what))


class Operand:
    """x1 (and x2) + prologue: see SISR_PRO_* in include/sisr_hip.h.  dims = logical (N,H,W,C)."""
    __slots__ = ('x1', 'x2', 'pa', 'pb', 'pd', 'ps', 'pt', 'mode', 'pro', 'slope', 'dims', 'x_out', 'fin')

    def __init__(self, x1, dims, pro=L.PRO_NONE, mode=L.X_NHWC, x2=None, pa=None, pb=None, pd=None,
                 ps=None, pt=None, slope=None):
        self.x1, self.x2, self.pa, self.pb, self.pd, self.ps, self.pt = x1, x2, pa, pb, pd, ps, pt
        self.mode, self.pro, self.slope, self.dims = mode, pro, slope, dims
        self.x_out = None
        self.fin = None                     # LazyBN whose scale / shift are this operand's pa / pd (deferred finalisation)

    @staticmethod
    def plain(t, dims=None, mode=L.X_NHWC):
        return Operand(t, dims or tuple(t.shape), mode=mode)

    @staticmethod
    def act(t, slope, dims=None):
        """lrelu(t, slope); slope: device scalar tensor (PReLU weight) or float."""
        return Operand(t, dims or tuple(t.shape), pro=L.PRO_ACT, slope=slope)

    @staticmethod
    def affine_act(t, scale, shift, slope=1.0):
        return Operand(t, tuple(t.shape), pro=L.PRO_AFFINE_ACT, pa=scale, pd=shift, slope=slope)

    @staticmethod
    def res_affine(res, res_slope, t, scale, shift, out):
        """lrelu(res, res_slope) + (scale*t + shift) -- a residual block's skip sum x + BN2(c2) (model_generator.py:19)
        formed in the consuming conv's staging; the conv also stores the sum to `out` (persistent trunk kernels only:
        ask trunk_takes_skip_sum() first)."""
        op = Operand(res, tuple(res.shape), pro=L.PRO_RES_AFFINE, x2=t, pa=scale, pd=shift, slope=res_slope)
        op.x_out = out
        return op

    def fill(self, d, g=False):
        """write this operand into a ConvDesc / WgradDesc (g=True: the output-gradient operand)"""
        names = (('g1', 'g2', 'qa', 'qb', 'qd', 'qs', 'qt', 'g_mode', 'gpro_mode', 'gpro_slope_p', 'gpro_slope')
                 if g else
                 ('x1', 'x2', 'pa', 'pb', 'pd', 'ps', 'pt', 'x_mode', 'pro_mode', 'pro_slope_p', 'pro_slope'))
        vals = (self.x1, self.x2, self.pa, self.pb, self.pd, self.ps, self.pt)
        for n, v in zip(names[:7], vals):
            setattr(d, n, _ptr(v))
        assert self.x2 is None or self.x2.dtype == self.x1.dtype, 'operand pair with mixed storage types'
        setattr(d, 'g_bf16' if g else 'x_bf16', _bf(self.x1))
        setattr(d, names[7], self.mode)
        setattr(d, names[8], self.pro)
        if not g and hasattr(d, 'x_out'):
            d.x_out = _ptr(self.x_out)
        for n, v in zip(names[9:], _slope(self.slope)):
            setattr(d, n, v)


def _conv_desc(n, h, w, cin, ho, wo, cout, kh, kw, stride, pad_y, pad_x, y_s=1, y_o=(0, 0), y_hw=None):
    """a ConvDesc of this geometry whose output pixel (a, b) is stored at (y_s a + y_o[0], y_s b + y_o[1]) of a y_hw image"""
    d = L.ConvDesc()
    d.N, d.H, d.W, d.Cin, d.Ho, d.Wo, d.Cout = n, h, w, cin, ho, wo, cout
    d.KH, d.KW, d.stride, d.pad_y, d.pad_x = kh, kw, stride, pad_y, pad_x
    d.y_sy = d.y_sx = y_s
    (d.y_oy, d.y_ox), (d.y_H, d.y_W) = y_o, y_hw or (ho, wo)
    return d


class ConvGeom:
    """Static geometry of one convolution + cached kernel plans per input shape."""

    def __init__(self, cin, cout, k, stride=1, pad=None, shuffle2=False, deep_dgrad=False):
        self.cin, self.cout, self.k, self.stride = cin, cout, k, stride
        self.pad = (k // 2) if pad is None else pad
        self.shuffle2 = shuffle2
        # trunk-shaped layers (3x3, 64 -> 64, stride 1) whose DATA GRADIENT never arrives with a BatchNorm-backward prologue
        # (the frozen VGG stack): the persistent trunk kernel refuses it, so it is planned for conv_deep.hip instead
        self.deep_dgrad = deep_dgrad
        # the data gradient of this layer never arrives through a BatchNorm-backward prologue (frozen VGG): its staging is
        # cheap, so the planner may pick the 64-cout tiles that plenty of pixel tiles favour (sisr_conv2d_deep_plan's prefer_bn)
        self.light_backward = deep_dgrad
        self._plans = {}

    def _deep_ok(self, role, h, w):
        """this role (0 forward, 1 data gradient) of the layer is planned for the split-K implicit-GEMM family (conv_deep.hip):
        bf16 tensors, 3x3, channels in 32s / 64s, no PixelShuffle store; the trunk geometry stays with the persistent trunk
        kernels wherever they take it (H % 8 == 0, W % 16 == 0)"""
        if PRECISION != 'bf16' or not storage_bf16() or not _on('SISR_DEEP'):
            return False
        if self.k != 3 or self.shuffle2:
            return False
        cin, cout = (self.cin, self.cout) if role == 0 else (self.cout, self.cin)
        if cin % 32 or cout % 64:
            return False
        trunk_shape = (self.cin == 64 and self.cout == 64 and self.stride == 1 and h % 8 == 0 and w % 16 == 0
                       and _on('SISR_TRUNK'))
        if trunk_shape and not (role == 1 and self.deep_dgrad):
            return False
        return True

    def out_hw(self, h, w):
        return ((h + 2 * self.pad - self.k) // self.stride + 1, (w + 2 * self.pad - self.k) // self.stride + 1)

    def _s2_class_plan(self, lib, n, h, w, ho, wo, py, px):
        khc, pady, r0y = _s2_taps(self.k, self.pad, py)
        kwc, padx, r0x = _s2_taps(self.k, self.pad, px)
        hc, wc = (h - py + 1) // 2, (w - px + 1) // 2
        if khc == 0 or kwc == 0 or hc <= 0 or wc <= 0:
            return None
        d = _conv_desc(n, ho, wo, self.cout, hc, wc, self.cin, khc, kwc, 1, pady, padx, y_s=2, y_o=(py, px), y_hw=(h, w))
        return S2Class(d, r0y, r0x, self._plan_conv(lib, d, 1, PRECISION == 'bf16', h, w, 'dgrad stride-2 class'))

    def _plan_conv(self, lib, d, role, want_bf16, h, w, what):
        """plan descriptor d (role 0 forward, 1 data gradient) for the best family that takes it -> Kind"""
        if not (want_bf16 and d.Cin % 32 == 0 and lib.sisr_conv2d_plan_bf16(C.byref(d)) == 0):
            L.check(lib.sisr_conv2d_plan(C.byref(d)), 'sisr_conv2d_plan(%s)' % what)
            return Kind.F32
        bn = 128 if role == 1 and not self.light_backward else 0
        if self._deep_ok(role, h, w) and lib.sisr_conv2d_deep_plan(C.byref(d), 0, bn, 1) == 0:
            return Kind.DEEP                                          # (its own weight image)
        return Kind.BF16

    def _s2_deep_plan(self, lib, n, h, w, ho, wo):
        """stride-2 data gradient as ONE conv_deep.hip launch over the four output-parity classes (even sizes): -> (descriptor of
        the 2 x 2-tap class convolution, [(taps y, taps x, R0y, R0x)] per class c = 2 py + px) or None"""
        if h % 2 or w % 2 or self.k != 3 or self.pad != 1 or not self._deep_ok(1, h, w):
            return None
        d = _conv_desc(n, ho, wo, self.cout, h // 2, w // 2, self.cin, 2, 2, 1, 0, 0, y_s=2, y_hw=(h, w))
        if (ho, wo) != (h // 2, w // 2) or lib.sisr_conv2d_plan_bf16(C.byref(d)) != 0:
            return None
        if lib.sisr_conv2d_deep_plan(C.byref(d), 0, 0 if self.light_backward else 128, 4) != 0:
            return None
        cls = []
        for py in (0, 1):
            for px in (0, 1):
                khc, pady, r0y = _s2_taps(self.k, self.pad, py)
                kwc, padx, r0x = _s2_taps(self.k, self.pad, px)
                assert pady == 0 and padx == 0 and khc <= 2 and kwc <= 2
                cls.append(S2Taps(khc, kwc, r0y, r0x))
        return d, cls

    def plans(self, n, h, w, max_pixel_blocks=512):
        """-> (fwd desc, dgrad desc | S2x4 | [4 x S2Class | None], wgrad desc, kinds) where kinds = (forward, data gradient, weight
        gradient) names the Kind each template was planned for.  (The four-class list reports Kind.F32 whatever its classes run on:
        each S2Class carries its own kind.)"""
        key = (n, h, w, PRECISION, storage_bf16(), max_pixel_blocks, _knob('SISR_DEEP', '1'), _knob('SISR_WGRAD_DEEP', '1'),
               _knob('SISR_WGRAD_DEEP_PB', ''))
        if key in self._plans:
            return self._plans[key]
        lib = L.lib()
        ho, wo = self.out_hw(h, w)
        f = _conv_desc(n, h, w, self.cin, ho, wo, self.cout, self.k, self.k, self.stride, self.pad, self.pad)
        f.y_mode = L.Y_SHUFFLE2 if self.shuffle2 else L.Y_NHWC
        want_bf16 = PRECISION == 'bf16' and self.k * self.k <= 9
        f_kind = self._plan_conv(lib, f, 0, want_bf16, h, w, 'fwd')
        d_kind = Kind.F32
        if self.stride == 1:
            pad = self.k - 1 - self.pad      # data gradient: conv over dy with flipped taps, roles swapped
            d = _conv_desc(n, ho, wo, self.cout, h, w, self.cin, self.k, self.k, 1, pad, pad)
            d_kind = self._plan_conv(lib, d, 1, want_bf16, h, w, 'dgrad')
        else:
            x4 = self._s2_deep_plan(lib, n, h, w, ho, wo) if want_bf16 else None
            if x4 is not None:
                d, d_kind = S2x4(*x4), Kind.DEEP_S2X4
            else:
                d = [self._s2_class_plan(lib, n, h, w, ho, wo, py, px) for py in (0, 1) for px in (0, 1)]
        g = L.WgradDesc()
        g.N, g.H, g.W, g.Cin, g.Ho, g.Wo, g.Cout = n, h, w, self.cin, ho, wo, self.cout
        g.KH = g.KW = self.k
        g.stride, g.pad_y, g.pad_x = self.stride, self.pad, self.pad
        g_kind = Kind.F32
        if want_bf16 and self.cin % 32 == 0:
            # few-channel outputs (the generator's 3-channel last conv): the bf16 kernel runs on the gradient
            # image padded to 4 channels (conv_wgrad materialises it), 16x the exact-fp32 matrix rate
            g.Cout = (self.cout + 3) // 4 * 4 if self.cout < 32 else self.cout
            if g.Cout % 4 == 0 and lib.sisr_wgrad_plan_bf16(C.byref(g), max_pixel_blocks) == 0:
                g_kind = Kind.BF16
                if self.k == 3 and self.pad == 1:
                    lib.sisr_wgrad_deep_plan(C.byref(g), 0)           # 3x3, channels in 64s: wgrad_deep.hip (g.deep.enabled)
        if g_kind == Kind.F32:
            g.Cout = self.cout
            L.check(lib.sisr_wgrad_plan(C.byref(g), max_pixel_blocks), 'sisr_wgrad_plan')
        g.slab_stride = g.slab_elems + g.CoutPad
        self._plans[key] = (f, d, g, (f_kind, d_kind, g_kind))
        return self._plans[key]


# one output-parity class c = 2 py + px of a stride-2 data gradient: as a stride-1 conv of its own (descriptor, Kind), or as its taps
# inside an S2x4 launch.  Forward tap (r, s) of class tap (r', s') is (r0y - 2 r', r0x - 2 s').
S2Class = namedtuple('S2Class', 'desc r0y r0x kind')
S2Taps = namedtuple('S2Taps', 'kh kw r0y r0x')


class S2x4:
    """the data gradient of a stride-2 layer planned as one conv_deep.hip launch over its four output-parity classes"""

    def __init__(self, desc, classes):
        self.desc, self.classes = desc, classes          # classes[c]: S2Taps, c = 2 py + px


DG_NONE, DG_CONV, DG_CLASSES, DG_X4 = 'none', 'conv', 'classes', 'x4'


def _dgrad_shape(d):
    """which of its shapes a data-gradient plan (ConvGeom.plans()[1]) has: DG_CONV one stride-1 conv, DG_X4 an S2x4, DG_CLASSES four
    S2Class | None, DG_NONE nothing planned"""
    if d is None or isinstance(d, S2x4):
        return DG_NONE if d is None else DG_X4
    return DG_CLASSES if isinstance(d, list) else DG_CONV


def _all_deep(classes):
    """every one of the four classes exists and runs on conv_deep.hip (whose epilogue can emit BatchNorm-backward partial rows)"""
    return all(c is not None and c.kind == Kind.DEEP for c in classes)


def _s2_taps(k, pad, parity):
    """stride-2 data gradient along one axis, output index 2a+parity: contributing dy index a+delta
    for forward taps r with (parity+pad-r) even.  -> (n_taps, pad', R0) with r = R0 - 2 r'."""
    deltas = sorted((parity + pad - r) // 2 for r in range(k) if (parity + pad - r) % 2 == 0)
    if not deltas:
        return 0, 0, 0
    return len(deltas), -deltas[0], parity + pad - 2 * deltas[0]


class ConvRef:
    """One convolution of a network: geometry + where its parameters / spectral-norm buffers live."""

    def __init__(self, geom, weight, bias, u=None, v=None):
        self.geom, self.weight, self.bias, self.u, self.v = geom, weight, bias, u, v


class Prepared:
    """Per-forward products of sisr_weights_prepare for one conv (kept for the backward pass)."""
    __slots__ = ('ref', 'plans', 'kinds', 'wpk_fwd', 'wpk_dgrad', 'sigma', 'inv_sigma', 'u_used', 'v_used', 'lanes', 'ldsimg')


def _trunk_ldsimg(gm, plan_f, plan_d, kinds):
    """(forward, data-gradient) mode of the LDS-order weight image of the fp32-tensor trunk conv (SISR_WIMG_F32's
    `extra`): 0 none, 1 fp32 values, 2 split pairs -- for 3x3 64 -> 64 convs on the fp32 kernels"""
    if gm.k != 3 or gm.cin != 64 or gm.cout != 64 or gm.stride != 1:
        return 0, 0
    mode = 2 if mfma_split() else 1

    def ok(desc, kind):
        return kind == Kind.F32 and desc.plan.CK == 32 and desc.plan.CoutPad == 64 and desc.plan.n_chunk == 2
    return (mode if ok(plan_f, kinds[0]) else 0), (mode if _dgrad_shape(plan_d) == DG_CONV and ok(plan_d, kinds[1]) else 0)


def _trunk_lanes(gm, plan_f, plan_d, kinds):
    """(forward, data-gradient): the bf16 weight buffer also gets the lane-order image of the persistent trunk kernels
    (SISR_WIMG_BF16's `extra`) -- only where those kernels can take the layer: 3x3, stride 1, 64 input channels,
    64 couts (or the 256 of the upscale conv) on the generic bf16 family (Kind.BF16, not the deep family)"""
    if gm.k != 3 or gm.stride != 1:
        return False, False
    lf = kinds[0] == Kind.BF16 and gm.cin == 64 and plan_f.plan.CK == 32 and plan_f.plan.CoutPad in (64, 256)
    ld = (kinds[1] == Kind.BF16 and _dgrad_shape(plan_d) == DG_CONV and gm.cout == 64 and gm.cin == 64
          and plan_d.plan.CK == 32 and plan_d.plan.CoutPad == 64)
    return lf, ld


_WEIGHT_EPOCH = [0]


def invalidate_weight_caches():
    """Packed weight images kept across forwards (prepare_weights(cache=...)) are valid only while the weights they were made from
    are: anything that changes parameters WITHOUT torch's version counter noticing calls this -- the fused Adam step (its kernel
    writes through raw pointers) and every HIP-graph capture / segment begin (an optimizer step the capture cannot see runs at
    the boundary when the graph is replayed, and the cached buffer of another capture is that graph's private memory)."""
    _WEIGHT_EPOCH[0] += 1


# one packed image of a layer: `slots` floats at `off` of buffer 'b' | 'd', written as its SisrWeightImage `rec` (dst unset) says
ImageSpec = namedtuple('ImageSpec', 'buf off slots rec')


def _image_rec(desc, kind, taps, transposed, ldsimg=0, lanes=False, row_taps=None):
    """the SisrWeightImage of one role of a layer: desc / kind the consumer's descriptor and Kind, taps = (KH', KW', R0y, Sy, R0x, Sx)
    its tap map (include/sisr_hip.h); ldsimg: the LDS-order mode, read for an fp32 image only; lanes: the lane-order copy, read for
    a bf16 image only; row_taps: taps per row of a conv_deep.hip image where they are not its own KW"""
    g = L.WeightImage()
    g.transposed = int(transposed)
    g.KH, g.KW, g.R0y, g.Sy, g.R0x, g.Sx = taps
    if Kind(kind).deep:
        g.format, g.CK, g.n_chunk, g.CoutPad, g.extra = L.WIMG_DEEP, 32, desc.Cin // 32, desc.Cout, row_taps or g.KW
    else:
        g.format, g.extra = (L.WIMG_BF16, int(bool(lanes))) if kind == Kind.BF16 else (L.WIMG_F32, int(ldsimg))
        for n in ('CK', 'PS', 'KROWP', 'n_chunk', 'CoutPad'):
            setattr(g, n, getattr(desc.plan, n))
    return g


def _layout_weights(items, need_dgrad):
    """Host-only pass of prepare_weights (no device call): per layer a Prepared with plans, kinds, lanes, ldsimg and offs[i] =
    (images, sigma block, power-iteration scratch): images[k] is the ImageSpec | None of SisrWeightDesc.img[k] -- the forward image,
    then the stride-1 data gradient or the four parity classes of a stride-2 one --, its length the library's own answer; the
    last two are offsets into 's'.  sizes: fp32 slots of 'b' (images rebuilt on every call), 'd' (conv_deep.hip's), 's'."""
    lib = L.lib()
    sizes = {'b': 0, 'd': 0, 's': 0}

    def take(buf, n):
        off = sizes[buf]
        sizes[buf] += _align4(n)                       # every piece starts on 16 bytes
        return (buf, off, n)

    def image(desc, kind, taps, transposed, **copy):
        rec = _image_rec(desc, kind, taps, transposed, **copy)
        nbytes = L.check_count(lib.sisr_weight_image_bytes(C.byref(rec)), 'sisr_weight_image_bytes')
        return ImageSpec(*take('d' if rec.format == L.WIMG_DEEP else 'b', (nbytes + 3) // 4), rec)
    preps, offs = [], []
    for ref, n, h, w in items:
        gm = ref.geom
        k = gm.k
        p = Prepared()
        f, d, g, p.kinds = gm.plans(n, h, w)
        p.ref, p.plans = ref, (f, d, g)
        p.lanes = _trunk_lanes(gm, f, d, p.kinds)
        p.ldsimg = _trunk_ldsimg(gm, f, d, p.kinds)
        imgs = [image(f, p.kinds[0], (k, k, 0, 1, 0, 1), False, ldsimg=p.ldsimg[0], lanes=p.lanes[0])] + [None] * 4
        shape = _dgrad_shape(d) if need_dgrad else DG_NONE
        if shape == DG_X4:
            imgs[1:] = [image(d.desc, Kind.DEEP, (t.kh, t.kw, t.r0y, -2, t.r0x, -2), True, row_taps=2) for t in d.classes]
        elif shape == DG_CLASSES:
            imgs[1:] = [c and image(c.desc, c.kind, (c.desc.KH, c.desc.KW, c.r0y, -2, c.r0x, -2), True) for c in d]
        elif shape == DG_CONV:
            imgs[1] = image(d, p.kinds[1], (k, k, k - 1, -1, k - 1, -1), True, ldsimg=p.ldsimg[1], lanes=p.lanes[1])
        rows, cols = gm.cout, gm.cin * gm.k * gm.k
        sn = ref.u is not None
        off_s = take('s', 4 + (_align4(rows) + _align4(cols) if sn else 0))[1]
        off_w = take('s', _align4((rows + 15) // 16 * cols + rows) if sn else 0)[1]     # power-iteration scratch: [ceil(rows/16)][cols] + [rows]
        preps.append(p)
        offs.append((imgs, off_s, off_w))
    return preps, offs, sizes


def _fill_weight_desc(t, p, off, bufs, training, deep_hit):
    """SisrWeightDesc `t` of one layer and the views of its Prepared `p`, from its layout record and the base tensors bufs['b' | 'd'
    | 's'].  deep_hit: the conv_deep.hip images are cached: not packed again (null pointers).  -> the layer has such an image"""
    imgs, off_s, off_w = off
    ref, gm, d = p.ref, p.ref.geom, p.plans[1]
    sm = bufs['s']
    views, has_deep = [None] * len(imgs), False
    for i, s in enumerate(imgs):
        if s is None:
            continue
        views[i] = bufs[s.buf][s.off:s.off + s.slots]
        t.img[i] = s.rec
        deep = s.rec.format == L.WIMG_DEEP
        has_deep |= deep
        if not (deep and deep_hit):
            t.img[i].dst = views[i].data_ptr()
    p.wpk_fwd = views[0]
    if all(s is None for s in imgs[1:]):               # (need_dgrad=False: no data-gradient image is packed)
        p.wpk_dgrad = None
    else:
        p.wpk_dgrad = views[1:] if _dgrad_shape(d) in (DG_X4, DG_CLASSES) else views[1]
    p.sigma = sm[off_s:off_s + 1]
    p.inv_sigma = sm[off_s + 1:off_s + 2]          # written next to sigma: the conv_deep.hip epilogue scale
    t.w_orig, t.sigma, t.wdp_scaled = ref.weight.data_ptr(), p.sigma.data_ptr(), 0
    t.Cout, t.Cin, t.KH, t.KW = gm.cout, gm.cin, gm.k, gm.k
    t.training, t.shuffle2 = int(training), int(gm.shuffle2)
    p.u_used = p.v_used = None
    if ref.u is not None:
        rows, cols = gm.cout, gm.cin * gm.k * gm.k
        t.sn_work = sm[off_w:].data_ptr()
        p.u_used = sm[off_s + 4:off_s + 4 + rows]
        p.v_used = sm[off_s + 4 + _align4(rows):off_s + 4 + _align4(rows) + cols]
        t.u, t.v = ref.u.data_ptr(), ref.v.data_ptr()
        t.u_used, t.v_used = p.u_used.data_ptr(), p.v_used.data_ptr()
    return has_deep


def prepare_weights(items, training, need_dgrad=True, cache=None):
    """items: [(ConvRef, n, h, w)].  Spectral-norm power iteration (in place on u/v when training), sigma, and the packed images
    for fwd and dgrad.  Images of the generic / trunk kernels hold W / sigma and are rebuilt on every call; the conv_deep.hip
    images (Kind.DEEP) hold W_orig itself -- those kernels apply 1 / sigma in their epilogue (Prepared.inv_sigma) -- so with `cache`
    (a dict owned by the module) they are packed once per optimizer step, not once per forward: the discriminator runs three
    forwards per SRGAN iteration, two of them on unchanged weights (train.py:132,156,174)."""
    lib = L.lib()
    dev = items[0][0].weight.device
    preps, offs, sizes = _layout_weights(items, need_dgrad)
    big = torch.empty(sizes['b'], dtype=torch.float32, device=dev)
    sm = torch.empty(sizes['s'], dtype=torch.float32, device=dev)
    deep, deep_hit = None, False
    if sizes['d']:
        key = (_WEIGHT_EPOCH[0], sizes['d'], need_dgrad, torch.cuda.is_current_stream_capturing(),
               tuple((id(ref.weight), ref.weight.data_ptr(), ref.weight._version, n, h, w) for ref, n, h, w in items))
        if cache is not None and cache.get('key') == key:
            deep, deep_hit = cache['deep'], True
        else:
            deep = torch.empty(sizes['d'], dtype=torch.float32, device=dev)
            if cache is not None:
                cache['key'], cache['deep'] = key, deep
    bufs = {'b': big, 'd': deep, 's': sm}
    table = (L.WeightDesc * len(items))()
    max_rows = max_cols = 1
    deep_cout = deep_cin = 0
    for t, p, off in zip(table, preps, offs):
        gm = p.ref.geom
        if _fill_weight_desc(t, p, off, bufs, training, deep_hit):
            deep_cout, deep_cin = max(deep_cout, gm.cout), max(deep_cin, gm.cin)
        max_rows, max_cols = max(max_rows, gm.cout), max(max_cols, gm.cin * gm.k * gm.k)
    tab_dev = _table_to_device(table, dev)
    # sigma must exist before any image that holds W / sigma is packed; weights without spectral norm get sigma = 1 from the
    # finishing kernel of the power iteration (one workgroup per weight) -- skipped only when nothing but cached images is left
    L.check(lib.sisr_weights_sn(tab_dev.data_ptr(), len(items), max_rows, max_cols, _stream()), 'sisr_weights_sn')
    if sizes['b']:
        L.check(lib.sisr_weights_pack(tab_dev.data_ptr(), len(items), max_rows, max_cols, _stream()), 'sisr_weights_pack')
    if sizes['d'] and not deep_hit:
        L.check(lib.sisr_weights_pack_deep(tab_dev.data_ptr(), len(items), deep_cout, deep_cin, _stream()), 'sisr_weights_pack_deep')
    return preps, (big, sm, tab_dev, deep)


_PIN_RING = {'buf': None, 'off': 0, 'half': 0, 'events': [[], []], 'streams': {}}
_PIN_CAPTURE = {'buf': None, 'off': 0}   # bump allocator for tables referenced by captured graphs
_PIN_KEEP = []                           # ... whose pinned storage must outlive every replay
_PIN_RING_BYTES = 4 << 20
_PIN_CAPTURE_CHUNK = 1 << 20


def reserve_capture_tables(nbytes):
    """Make sure the pinned staging area for descriptor tables of CAPTURED launches has `nbytes` free -- called by
    graph.GraphedStep BEFORE capture_begin with what its warm-up runs consumed: a pinned host allocation inside a
    stream capture invalidates the capture (hipHostMalloc is not capturable), so the bump allocator must never have to
    grow while one is running."""
    cap = _PIN_CAPTURE
    if cap['buf'] is None or cap['off'] + nbytes > cap['buf'].numel():
        assert not torch.cuda.is_current_stream_capturing()
        cap['buf'] = torch.empty(max(nbytes, _PIN_CAPTURE_CHUNK), dtype=torch.uint8, pin_memory=True)
        cap['off'] = 0
        _PIN_KEEP.append(cap['buf'])


_TABLE_BYTES = [0]                       # bytes of tables staged so far (GraphedStep sizes its reservation from the delta)


def table_bytes_staged():
    return _TABLE_BYTES[0]


def _fill_block_starts(table):
    """The block mapping of the multi-tensor launches (csrc/optim.hip) for a ctypes table (AdamDesc / EmaDesc rows) whose
    ``numel`` fields are set: every row's ``block_start`` = the blocks of the rows before it.  Returns the total."""
    lib, blocks = L.lib(), 0
    for row in table:
        row.block_start = blocks
        blocks += lib.sisr_adam_blocks(row.numel)
    return blocks


def _table_to_device(table, dev):
    """Descriptor table -> device without a host synchronisation: staged in pinned memory and copied
    asynchronously on the current stream.  Eager mode uses a 4 MB pinned ring in two halves: when a half is full an
    event is recorded on EVERY stream that issued copies out of it (tables are also uploaded from warm-up side streams
    and from the capture stream), and the host waits for those events before it writes into the half again (normally
    long complete: a half holds thousands of tables), so a slot is never rewritten while its copy may still be pending
    however far the GPU lags behind the host.  Under HIP-graph capture every table gets its own slice of a pinned
    bump buffer that is kept alive forever, because the captured copy node re-reads it on each replay; GraphedStep
    reserves that buffer before the capture begins (reserve_capture_tables)."""
    raw = bytes(table)
    n = (len(raw) + 255) & ~255
    _TABLE_BYTES[0] += n
    if torch.cuda.is_current_stream_capturing():
        cap = _PIN_CAPTURE
        if cap['buf'] is None or cap['off'] + n > cap['buf'].numel():
            # not reserved (a caller capturing without GraphedStep): the allocation below invalidates the capture on
            # ROCm 7.2 -- say why instead of failing later with a generic capture error
            raise RuntimeError('descriptor-table staging exhausted inside a stream capture: call '
                               'engine.reserve_capture_tables(nbytes) before capture_begin (GraphedStep does)')
        host = cap['buf'][cap['off']:cap['off'] + n]
        cap['off'] += n
        host[:len(raw)].copy_(torch.frombuffer(bytearray(raw), dtype=torch.uint8))
        return host.to(dev, non_blocking=True)
    ring = _PIN_RING
    if ring['buf'] is None:
        ring['buf'] = torch.empty(_PIN_RING_BYTES, dtype=torch.uint8, pin_memory=True)
        reserve_capture_tables(_PIN_CAPTURE_CHUNK)                          # allocated OUTSIDE capture
    half_bytes = _PIN_RING_BYTES // 2
    assert n <= half_bytes, 'descriptor table larger than half the pinned ring'
    if ring['off'] + n > (ring['half'] + 1) * half_bytes:          # this half is full: fence it, move to the other
        evs = []
        for st in ring['streams'].values():                         # every stream that copied out of the full half
            ev = torch.cuda.Event()
            ev.record(st)
            evs.append(ev)
        ring['events'][ring['half']] = evs
        ring['streams'] = {}
        ring['half'] ^= 1
        ring['off'] = ring['half'] * half_bytes
        for ev in ring['events'][ring['half']]:
            ev.synchronize()                                        # copies out of the half we are about to rewrite
        ring['events'][ring['half']] = []
    host = ring['buf'][ring['off']:ring['off'] + n]
    ring['off'] += n
    host[:len(raw)].copy_(torch.frombuffer(bytearray(raw), dtype=torch.uint8))
    cur = torch.cuda.current_stream()
    ring['streams'][cur.cuda_stream] = cur
    return host.to(dev, non_blocking=True)


def _alloc_out(n, ho, wo, c, y_mode, dev, res=None, alloc=torch.empty):
    """the output tensor of a conv with `c` output channels over n x ho x wo pixels, by store mode"""
    if y_mode == L.Y_NCHW:
        return alloc((n, c, ho, wo), dtype=torch.float32, device=dev)
    if y_mode == L.Y_SHUFFLE2:
        return alloc((n, 2 * ho, 2 * wo, c // 4), dtype=act_dtype(c // 4), device=dev)
    return alloc((n, ho, wo, c), dtype=act_dtype(c) if res is None else res.dtype, device=dev)


def _bind(d, kind, prep, op, image, bias, res, out):
    """operand, weight image, epilogue tensors and output of one conv launch.  A descriptor planned for conv_deep.hip gets that
    family's weight image (instead of `wpk`), the 1 / sigma its epilogue applies (the image holds W_orig) and a split workspace
    -> that workspace or None (the caller keeps it alive until the launch)"""
    assert tuple(op.dims) == (d.N, d.H, d.W, d.Cin), (op.dims, (d.N, d.H, d.W, d.Cin))
    op.fill(d)
    d.wpk, d.bias, d.res, d.y = image.data_ptr(), _ptr(bias), _ptr(res), out.data_ptr()
    d.y_bf16, d.res_bf16 = _bf(out), _bf(res)
    ws = None
    if kind.deep:
        d.wdeep, d.wpk = image.data_ptr(), None
        d.epi_scale_p = prep.inv_sigma.data_ptr()
        if d.deep.ws_bytes > 0:
            ws = torch.empty((d.deep.ws_bytes // 4,), dtype=torch.float32, device=out.device)
            d.deep_ws = ws.data_ptr()
    return ws


def _launch_conv(d, kind, what):
    fn = _entry(kind.bf16, 'conv')
    L.check(fn(C.byref(d), _stream()), '%s(%s)' % (fn.__name__, what))


def conv_forward(prep, op, bias=None, y_mode=None, epi=L.EPI_NONE, stats=False, res=None, out=None):
    """Launch the forward conv of `prep` on lazy operand `op`.  Returns (y, stat_part, cnt_part)."""
    f, kind = _copy_struct(prep.plans[0]), prep.kinds[0]
    gm = prep.ref.geom
    if y_mode is not None:
        f.y_mode = y_mode
    dev = op.x1.device
    if out is None:
        out = _alloc_out(f.N, f.Ho, f.Wo, gm.cout, f.y_mode, dev, res)
    ws = _bind(f, kind, prep, op, prep.wpk_fwd, bias, res, out)
    f.epi_act = epi
    f.mfma_split = mfma_split()
    f.plan.variant = int(prep.lanes[0]) | (2 * prep.ldsimg[0])           # bit 0: lane-order bf16 image; bits 1-2: LDS-order fp32 image (mode)
    fin = op.fin
    if fin is not None and not fin.done:
        # deferred BatchNorm finalisation: by this conv when it runs on a persistent trunk kernel, else stand-alone first
        fin.fill(f)
        if _on('SISR_FUSE_BNFIN') and not kind.deep and _entry(kind.bf16, 'trunk_eligible')(C.byref(f)) == 1:
            fin.done = True
        else:
            f.fin_stat = None
            fin.ensure()
    sp = cp = None
    if stats:
        # rows of the statistics partials: one per tile, or one per workgroup on the persistent trunk kernel.  The row
        # count depends on which kernel takes the descriptor, and that depends on the fusions requested (the upscale
        # variant of the trunk kernel has no statistics epilogue): ask with the statistics pointers already non-null
        f.stat_part = f.cnt_part = f.y
        rows = _entry(kind.bf16, 'parts')(C.byref(f))
        sp = torch.empty((rows, 2, gm.cout), dtype=torch.float32, device=dev)
        cp = torch.empty((rows,), dtype=torch.float32, device=dev)
        f.stat_part, f.cnt_part = sp.data_ptr(), cp.data_ptr()
    _launch_conv(f, kind, 'fwd')
    return out, sp, cp


def trunk_takes_skip_sum(prep, res, t):
    """the forward conv of `prep` runs on a persistent trunk kernel that can form the skip sum lrelu(res) + BN(t) in its
    staging (Operand.res_affine); SISR_FUSE_SKIP=0 keeps the separate elementwise pass"""
    if not _on('SISR_FUSE_SKIP') or res.dtype != t.dtype or tuple(res.shape) != tuple(t.shape):
        return False
    f = _copy_struct(prep.plans[0])
    if (f.N, f.H, f.W, f.Cin) != tuple(res.shape):
        return False
    f.x1 = f.x2 = f.x_out = f.pa = f.pd = f.wpk = f.y = res.data_ptr()         # (non-null placeholders: eligibility only)
    f.pro_mode = L.PRO_RES_AFFINE
    f.x_bf16 = f.y_bf16 = _bf(res)
    return _entry(prep.kinds[0].bf16, 'trunk_eligible')(C.byref(f)) == 1


def can_fuse_bn_backward(prep):
    """the data-gradient conv of `prep` can also emit the backward reductions of the BatchNorm its output feeds"""
    d, kind = prep.plans[1], prep.kinds[1]
    shape = _dgrad_shape(d)
    if shape != DG_CONV:                          # stride 2: one launch, or four parity classes all on the deep family
        return shape == DG_X4 or (shape == DG_CLASSES and _all_deep(d))
    if kind.deep:                                 # conv_deep.hip: any number of cout tiles
        return True
    if kind == Kind.F32:
        # fp32 build: only the persistent trunk kernel (conv_trunk_f32.hip) has that epilogue: ask the library with a probe.
        # conv_dgrad() falls back to the plain launch (and returns no partial rows) when the filled descriptor is not eligible
        p = _copy_struct(d)
        p.x1 = p.x2 = p.wpk = p.y = p.bnb_x = p.bnb_part = 1                        # (non-null placeholders: eligibility only)
        p.pro_mode = L.PRO_BNBWD
        return _entry(False, 'bnb_parts')(C.byref(p)) > 0
    return d.plan.variant == 0 and d.plan.CoutPad == d.plan.nsub * 32        # generic bf16 kernel: one cout tile


def _attach_bnb(descs, bnb, out):
    """BatchNorm-backward epilogue of the data-gradient launches descs = [(descriptor, Kind)] whose output `out` is the gradient
    arriving at BatchNorm(x), bnb = (x, consts, slope | None).  -> the partial rows for bn_backward(part=...), one block of rows
    per descriptor in the order given -- or None where the kernel that takes the descriptor has no such epilogue (the fusion
    is taken back then)"""
    x, consts, slope = bnb
    assert tuple(x.shape) == tuple(out.shape)
    rows = []
    for d, kind in descs:
        d.bnb_x, d.bnbx_bf16 = x.data_ptr(), _bf(x)
        d.bnb_part = d.y                            # (any non-null value: the row count depends on the fusions requested)
        rows.append(_entry(kind.bf16, 'bnb_parts')(C.byref(d)))
    if sum(rows) <= 0:                              # fp32 build, descriptor not taken by the persistent kernel: no fusion
        for d, _ in descs:
            d.bnb_x, d.bnb_part = None, None
        return None
    part = torch.empty((sum(rows), 2 * out.shape[-1] + 1), dtype=torch.float32, device=out.device)
    r0 = 0
    for (d, _), nr in zip(descs, rows):
        d.bnb_part = part[r0:].data_ptr()
        r0 += nr
        d.bnb_scale, d.bnb_shift, d.bnb_mean, d.bnb_invstd = (consts[0].data_ptr(), consts[1].data_ptr(),
                                                              consts[2].data_ptr(), consts[3].data_ptr())
        d.bnb_act = 0 if slope is None else 1
        d.bnb_slope_p, d.bnb_slope = _slope(slope)
    return part


def _launch_dgrad(descs, out, bnb, what):
    """the launches of one data gradient in order, with the BatchNorm-backward epilogue when bnb is given -> (out, partial rows)"""
    part = _attach_bnb(descs, bnb, out) if bnb is not None else None
    for d, kind in descs:
        _launch_conv(d, kind, what)
    return out, part


def _dgrad_x4(prep, dy_op, res, y_mode, bnb):
    """stride 2, one launch over the four output-parity classes (conv_deep.hip)"""
    x4, f, gm = prep.plans[1], prep.plans[0], prep.ref.geom
    d = _copy_struct(x4.desc)
    assert y_mode == L.Y_NHWC
    dev = dy_op.x1.device
    out = _alloc_out(f.N, f.H, f.W, gm.cin, y_mode, dev)
    ws = _bind(d, Kind.DEEP_S2X4, prep, dy_op, prep.wpk_dgrad[3], None, res, out)
    for c, buf in enumerate(prep.wpk_dgrad):
        d.wdeep_c[c], d.deep_ckh[c] = buf.data_ptr(), x4.classes[c].kh
    return _launch_dgrad([(d, Kind.DEEP_S2X4)], out, bnb, 'dgrad s2 x4')


def _dgrad_classes(prep, dy_op, res, y_mode, bnb):
    """stride 2: four output-parity classes, one launch each in class order"""
    classes, f, gm = prep.plans[1], prep.plans[0], prep.ref.geom
    assert y_mode == L.Y_NHWC
    dev = dy_op.x1.device
    complete = all(c is not None for c in classes)
    out = _alloc_out(f.N, f.H, f.W, gm.cin, y_mode, dev, alloc=torch.empty if complete else torch.zeros)
    descs, keep = [], []
    for c, buf in zip(classes, prep.wpk_dgrad):
        if c is None:
            continue
        d = _copy_struct(c.desc)
        keep.append(_bind(d, c.kind, prep, dy_op, buf, None, res, out))
        descs.append((d, c.kind))
    # fused BatchNorm-backward reductions: every class of the deep family emits the partial rows of ITS quarter of the pixels
    return _launch_dgrad(descs, out, bnb if _all_deep(classes) else None, 'dgrad s2')


def _dgrad_conv(prep, dy_op, res, y_mode, bnb):
    """stride 1: one conv over dy with the flipped weights"""
    d, kind, gm = _copy_struct(prep.plans[1]), prep.kinds[1], prep.ref.geom
    dev = dy_op.x1.device
    d.y_mode = y_mode
    out = _alloc_out(d.N, d.Ho, d.Wo, gm.cin, y_mode, dev, res)
    ws = _bind(d, kind, prep, dy_op, prep.wpk_dgrad, None, res, out)
    d.mfma_split = mfma_split()
    d.plan.variant = int(prep.lanes[1]) | (2 * prep.ldsimg[1])
    assert bnb is None or y_mode == L.Y_NHWC
    return _launch_dgrad([(d, kind)], out, bnb, 'dgrad')


_DGRAD = {DG_X4: _dgrad_x4, DG_CLASSES: _dgrad_classes, DG_CONV: _dgrad_conv}


def conv_dgrad(prep, dy_op, res=None, y_mode=L.Y_NHWC, bnb=None):
    """Data gradient: conv over the (lazy) output gradient with the flipped packed weights.
    bnb = (x, consts [4,C], slope | None): the result is the gradient arriving at BatchNorm(x) (through a leaky
    activation when slope is given); returns (out, partial rows for bn_backward_finalize) in that case."""
    out, part = _DGRAD[_dgrad_shape(prep.plans[1])](prep, dy_op, res, y_mode, bnb)
    return out if bnb is None else (out, part)


KERNEL_COUNTS = {}          # launches per kernel family, for the tests that must see a family run (not a timing path: host counters)


def _count(key, n=1):
    KERNEL_COUNTS[key] = KERNEL_COUNTS.get(key, 0) + n


# one fixed-order sum of per-workgroup slabs: red[i] = sum_s slab[s][i], i < stride; lead: the leading elements of every row stored as bf16
SlabJob = namedtuple('SlabJob', 'slab red n_slabs stride lead')


def _reduce_slabs(job):
    """the sum of one SlabJob in a launch of its own"""
    L.check(L.lib().sisr_slab_reduce_f32(job.slab.data_ptr(), job.red.data_ptr(), job.n_slabs, job.stride, job.lead, _stream()),
            'sisr_slab_reduce_f32')


class PendingSlabs:
    """Slab reductions that have not been launched yet.  conv_wgrad(..., defer=pending) leaves the fixed-order sum of
    its per-workgroup slabs here instead of launching sisr_slab_reduce_f32; the next bn_backward(..., part=rows,
    slabs=pending) carries one of them in ITS launch (sisr_bn_bwd_finalize_slab: the two jobs are independent and
    adjacent in a residual block's backward schedule -- one launch instead of two), and flush() launches whatever is
    left the ordinary way.  The reduced buffers are valid in stream order after either."""

    def __init__(self):
        self.jobs = []                      # SlabJob

    def pop(self):
        return self.jobs.pop(0) if self.jobs else None

    def flush(self):
        """whatever is left, in ONE launch per eight jobs (sisr_slab_reduce_multi: the jobs travel in the kernel arguments)"""
        if not self.jobs:
            return
        jobs, self.jobs = self.jobs, []
        n = len(jobs)
        slabs = (C.c_void_p * n)(*[j.slab.data_ptr() for j in jobs])
        outs = (C.c_void_p * n)(*[j.red.data_ptr() for j in jobs])
        counts = (C.c_int32 * n)(*[j.n_slabs for j in jobs])
        elems = (C.c_int64 * n)(*[j.stride for j in jobs])
        leads = (C.c_int64 * n)(*[j.lead for j in jobs])
        L.check(L.lib().sisr_slab_reduce_multi(C.addressof(slabs), C.addressof(outs), C.addressof(counts), C.addressof(elems),
                                               C.addressof(leads), n, _stream()), 'sisr_slab_reduce_multi')


# One weight gradient, prepared ONCE: g, the copy of the planned WgradDesc with both operands and mfma_split filled in; the operands
# themselves (their tensors stay alive until the launch); red, the buffer the reduced gradient WILL be in; route, the kernel family
# (L.ROUTE_*) the library's dispatcher sends g to -- asked here and nowhere else.  Whoever launches it (alone: _launch_wgrad; with
# others: WgradDeepBatch) binds the slabs.
WgradLaunch = namedtuple('WgradLaunch', 'prep g x_op dy_op red route')


def _wgrad_launch(prep, x_op, dy_op):
    g, bf16 = _copy_struct(prep.plans[2]), prep.kinds[2].bf16
    assert tuple(x_op.dims) == (g.N, g.H, g.W, g.Cin) and tuple(dy_op.dims) == (g.N, g.Ho, g.Wo, prep.ref.geom.cout), \
        (x_op.dims, dy_op.dims)
    x_op.fill(g)
    dy_op.fill(g, g=True)
    g.mfma_split = mfma_split()
    red = torch.empty((g.slab_stride,), dtype=torch.float32, device=x_op.x1.device)
    return WgradLaunch(prep, g, x_op, dy_op, red, _entry(bf16, 'wgrad_route')(C.byref(g)))


def _bind_slabs(w, n_slabs):
    """the [n_slabs, slab_stride] slab tensor of weight gradient w, bound to its descriptor (a row: one workgroup's gradient part, then its
    bias row) -> the SlabJob that sums it; its lead: what the launch of w.g stores as bf16 (the persistent and the deep bf16 kernels)"""
    g = w.g
    slab = torch.empty((n_slabs, g.slab_stride), dtype=torch.float32, device=w.red.device)
    g.slab = slab.data_ptr()
    g.bias_slab = slab.data_ptr() + 4 * g.slab_elems
    lead = int(_entry(True, 'slab_lead')(C.byref(g))) if w.prep.kinds[2].bf16 else 0
    return SlabJob(slab, w.red, n_slabs, g.slab_stride, lead)


def _launch_wgrad(w, defer=None):
    """weight gradient w in a launch of its own -> w.red"""
    g, dy_op, bf16, cout = w.g, w.dy_op, w.prep.kinds[2].bf16, w.prep.ref.geom.cout
    if g.Cout != cout and w.route != L.ROUTE_TOIMAGE:
        # the generator's last conv (64 -> 3) where the kernel that reads the NCHW image gradient itself (wgrad_toimage.hip) does not take
        # it: the bf16 kernel on a channel-padded NHWC copy of the gradient
        if dy_op.mode != L.X_NCHW or dy_op.pro not in (L.PRO_NONE, L.PRO_TANH_BWD):
            raise RuntimeError('padded weight gradient: NCHW gradient with no / tanh-backward prologue expected')
        g4 = torch.empty((g.N, g.Ho, g.Wo, g.Cout), dtype=torch.float32, device=w.red.device)
        L.check(L.lib().sisr_nchw_grad_to_nhwc4(dy_op.x1.data_ptr(), _ptr(dy_op.x2) if dy_op.pro == L.PRO_TANH_BWD else None,
                                                g4.data_ptr(), g.N, cout, g.Ho, g.Wo, g.Cout, _stream()), 'sisr_nchw_grad_to_nhwc4')
        Operand.plain(g4).fill(g, g=True)
    if w.route == L.ROUTE_DEEP:
        _count('wgrad_deep')
    job = _bind_slabs(w, _entry(bf16, 'slabs')(C.byref(g)))
    fn = _entry(bf16, 'wgrad')
    L.check(fn(C.byref(g), _stream()), fn.__name__)
    if defer is not None and _on('SISR_FUSE_SLABRED'):
        defer.jobs.append(job)
    else:
        _reduce_slabs(job)
    return w.red


def conv_wgrad(prep, x_op, dy_op, defer=None):
    """Weight + bias gradient in packed layout: returns the reduced [slab_elems + CoutPad] buffer.
    defer (PendingSlabs or None): leave the slab reduction to a later launch (see PendingSlabs)."""
    return _launch_wgrad(_wgrad_launch(prep, x_op, dy_op), defer)


def _toimage_bwd_desc(prep, x_op, dy_op):
    """the SisrToImageBwdDesc of the generator's last conv `prep` for x_op = lrelu(pre, slope) and the NCHW image gradient dy_op
    (outputs unbound): geometry and slab layout from the planned weight gradient, the weight image's layout from the forward plan"""
    g, f = prep.plans[2], prep.plans[0].plan
    d = L.ToImageBwdDesc()
    for n in ('N', 'H', 'W', 'Cin', 'Cout', 'KH', 'KW', 'stride', 'pad_y', 'pad_x', 'CK', 'PS', 'KROWP', 'n_chunk', 'CoutPad',
              'slab_elems', 'slab_stride'):
        setattr(d, n, getattr(g, n))
    d.w_CK, d.w_PS, d.w_KROWP, d.w_CoutPad = f.CK, f.PS, f.KROWP, f.CoutPad
    d.pre, d.pre_bf16 = x_op.x1.data_ptr(), _bf(x_op.x1)
    d.g_bf16 = int(act_dtype(g.Cin) == torch.bfloat16)
    d.slope_p, d.slope = _slope(x_op.slope)
    d.dy, d.out = dy_op.x1.data_ptr(), _ptr(dy_op.x2) if dy_op.pro == L.PRO_TANH_BWD else None
    d.wpk = prep.wpk_fwd.data_ptr()
    return d


def toimage_backward(prep, x_op, dy_op, defer=None):
    """The whole backward of the generator's last conv in one launch (toimage_bwd.hip): x_op = lrelu(pre, slope), the lazy activation
    of the last upscale stage; dy_op = the NCHW image gradient (prologue none / tanh-backward).  -> (g, dslope, red): the gradient wrt
    the activated input, the gradient of `slope` [1] and the buffer the reduced packed weight gradient WILL be in (its slabs are bound
    and their sum launched or deferred exactly as _launch_wgrad does) -- or None where the kernel does not take the layer (an odd
    shape, bf16 tensors, SISR_TOIMAGE_BWD=0): the caller keeps conv_wgrad + conv_dgrad + prelu_slope_grad."""
    lib = L.lib()
    if any(k.bf16 for k in prep.kinds) or _dgrad_shape(prep.plans[1]) != DG_CONV:
        return None
    if x_op.pro != L.PRO_ACT or x_op.mode != L.X_NHWC or dy_op.mode != L.X_NCHW or dy_op.pro not in (L.PRO_NONE, L.PRO_TANH_BWD):
        return None
    d = _toimage_bwd_desc(prep, x_op, dy_op)
    if tuple(x_op.dims) != (d.N, d.H, d.W, d.Cin) or lib.sisr_toimage_bwd_f32_eligible(C.byref(d)) != 1:
        return None
    w = _wgrad_launch(prep, x_op, dy_op)
    job = _bind_slabs(w, L.check_count(lib.sisr_toimage_bwd_f32_parts(C.byref(d)), 'sisr_toimage_bwd_f32_parts'))
    dev = w.red.device
    g = torch.empty(tuple(x_op.dims), dtype=torch.float32, device=dev)
    part = torch.empty((job.n_slabs,), dtype=torch.float64, device=dev)
    dslope = torch.empty((1,), dtype=torch.float32, device=dev)
    d.slab, d.bias_slab, d.g = w.g.slab, w.g.bias_slab, g.data_ptr()
    d.dslope_part, d.dslope = part.data_ptr(), dslope.data_ptr()
    L.check(lib.sisr_toimage_bwd_f32(C.byref(d), _stream()), 'sisr_toimage_bwd_f32')
    _count('toimage_bwd')
    if defer is not None and _on('SISR_FUSE_SLABRED'):
        defer.jobs.append(job)
    else:
        _reduce_slabs(job)
    return g, dslope, w.red


def _deep_batch_key(g):
    """members of one sisr_wgrad_deep_batch launch share the stride (a template argument) and whether the gradient prologue reads
    a second tensor -- the library checks operand_needs_x2(gpro_mode) of every member against the first's"""
    return g.stride, g.gpro_mode in (L.PRO_BNBWD, L.PRO_BNACT_BWD, L.PRO_ACT_BWD)


def _trunk_batch_key(prep, g):
    """members of one sisr_wgrad_trunk(_f32)_batch launch share the tensor family (the entry point) and the gradient prologue
    itself -- the library's wtrunk_batch_check compares every member's gpro_mode with the first's"""
    return prep.kinds[2].bf16, g.gpro_mode


def _batch_table(group, n_slabs, pending):
    """the descriptor table of one batched launch, every member's n_slabs(g) slabs bound to it and their sums left with `pending`"""
    table = (L.WgradDesc * len(group))()
    for i, w in enumerate(group):
        pending.jobs.append(_bind_slabs(w, n_slabs(w.g)))
        table[i] = w.g
    return table


def _grouped(members, key):
    groups = {}
    for w in members:
        groups.setdefault(key(w), []).append(w)
    return groups


class WgradDeepBatch:
    """Weight gradients of the layers that run on wgrad_deep.hip, collected during a backward pass and launched TOGETHER (one launch
    per stride: grid z = layer).  Nothing consumes a weight gradient before the optimizer step, so a schedule may hold them back;
    at 96 x 96 a layer alone spreads 4 tiles per workgroup over the chip and pays ~15 us of prologue and slab stores for ~6 us of
    work, while a batch plans every member for its SHARE of the chip: 3-4 times the tiles per workgroup behind the same fixed costs,
    a third of the slabs.  add() returns the buffer the reduced gradient WILL be in -- valid after run(pending) and pending.flush()."""

    def __init__(self):
        self.items = []                 # WgradLaunch
        self.trunk = []                 # layers the persistent trunk kernel keeps (LR 96): batched per gradient-prologue kind

    def add(self, prep, x_op, dy_op):
        """-> reduced-gradient buffer, or None when the layer does not qualify (the caller then runs conv_wgrad as usual)"""
        return self.offer(_wgrad_launch(prep, x_op, dy_op))

    def offer(self, w):
        """-> w.red, or None when weight gradient w (a WgradLaunch) does not qualify (the caller then launches it: _launch_wgrad).  Which
        list keeps it follows from the build, its route and wgrad_deep.hip's own answer"""
        g, members = w.g, self.items
        plain_trunk = w.route == L.ROUTE_TRUNK and g.Cout == 64      # (what the batched trunk kernels take: not the upscale conv)
        if not _on('SISR_WGRAD_BATCH'):
            return None
        if not w.prep.kinds[2].bf16:
            # fp32-tensor builds: the persistent trunk kernel's plain layers are batched like the bf16 build's
            if not plain_trunk or g.g_mode != L.X_NHWC:
                return None
            members = self.trunk
        elif w.route == L.ROUTE_TOIMAGE or not L.lib().sisr_wgrad_deep_eligible(C.byref(g)):
            return None
        # the persistent trunk kernel keeps a layer where its 8 x 16 tiles fill the chip -- at LR 48 they are 288 for 256 CUs: 144 workgroups
        # of two, and the batch measured 366 us for the 33 trunk layers against 33 x 16.5 us (sisr_wgrad_bf16_slab_lead then answers for
        # the trunk kernel: the same SISR_SLAB_BF16 rule as wgrad_deep.hip's) -- and its launches are batched too (_run_trunk)
        elif w.route == L.ROUTE_TRUNK and (g.N * g.H * g.W >= int(_knob('SISR_WGRAD_BATCH_TRUNK_PIXELS', 384 * 128))
                                           or not _on('SISR_WGRAD_BATCH_TRUNK')):
            if not plain_trunk:
                return None
            members = self.trunk
        members.append(w)
        return w.red

    def run(self, pending):
        """launch what was collected; the slab sums are left with `pending` (PendingSlabs: the caller flushes it)"""
        self._run_trunk(pending)
        lib = L.lib()
        items, self.items = self.items, []
        for group in _grouped(items, lambda w: _deep_batch_key(w.g)).values():
            work = [float(w.g.N) * w.g.Ho * w.g.Wo * w.g.Cin * w.g.Cout for w in group]
            tot = sum(work)
            first_wg = 0
            for w, wk in zip(group, work):
                g = w.g
                if len(group) > 1:
                    blocks = (g.Cin // 64) * (g.Cout // 64)
                    share = max(blocks, int(round(256.0 * wk / tot)))
                    cache, key = w.prep.ref.geom._plans, ('wgrad_deep_share', g.N, g.H, g.W, share, _knob('SISR_SLAB_BF16', '1'))
                    if key not in cache:
                        t = _copy_struct(g)
                        L.check(lib.sisr_wgrad_deep_plan(C.byref(t), share), 'sisr_wgrad_deep_plan(share)')
                        cache[key] = _copy_struct(t.deep)
                    g.deep = cache[key]
                g.deep.batch_first_wg = first_wg
                first_wg += g.deep.n_cib * g.deep.n_cob * g.deep.n_pb
            table = _batch_table(group, lambda g: g.deep.n_pb, pending)
            dev = _table_to_device(table, group[0].red.device)
            L.check(lib.sisr_wgrad_deep_batch(table, dev.data_ptr(), len(group), _stream()), 'sisr_wgrad_deep_batch')
            _count('wgrad_deep', len(group))
            _count('wgrad_deep_batch')

    def _run_trunk(self, pending):
        items, self.trunk = self.trunk, []
        for (is_bf16, _), group in _grouped(items, lambda w: _trunk_batch_key(w.prep, w.g)).items():
            n = len(group)
            # 256 workgroup slots over the layers: every workgroup walks its share of ONE layer's tiles back to back (17 layers of 1,152
            # tiles: 15 workgroups x 77; alone, a layer is 231 workgroups x 5 with a tenth of the chip idle)
            wpl = max(1, min(256 // n, 231))
            table = _batch_table(group, lambda g: wpl, pending)
            args = (C.c_char * (n * _entry(is_bf16, 'batch_arg_bytes')()))()
            f_args, f_run = _entry(is_bf16, 'batch_args'), _entry(is_bf16, 'batch')
            L.check(f_args(table, n, C.addressof(args)), f_args.__name__)
            dev = _table_to_device(args, group[0].red.device)
            L.check(f_run(table, dev.data_ptr(), n, wpl, _stream()), f_run.__name__)
            _count('wgrad_trunk_batch')


# a reduced packed gradient waiting to be un-packed into the gradients of its layer's weight and bias
GradItem = namedtuple('GradItem', 'prep red want_w want_b')


class WeightGradBatch:
    """Collects (prepared conv, reduced packed gradient) pairs; one launch un-packs them all."""

    def __init__(self):
        self.items = []                 # GradItem

    def add(self, prep, red, want_w=True, want_b=True):
        self.items.append(GradItem(prep, red, want_w, want_b))

    def run(self):
        """returns {id(ConvRef): (grad_w or None, grad_b or None)}"""
        if not self.items:
            return {}
        # 3x3 layers whose gradient slabs come from the bf16 kernels (layout 1) with channels in 32s take the whole-tile
        # un-packing (sisr_weights_grad_fast); the rest (9x9 / 3-channel / fp32-slab layers) the generic pair
        fast, slow = [], []
        for it in self.items:
            gm, g = it.prep.ref.geom, it.prep.plans[2]
            ok = (it.prep.kinds[2].bf16 and gm.k == 3 and gm.cin % 32 == 0 and gm.cout % 32 == 0 and not gm.shuffle2
                  and g.CoutPad >= gm.cout)
            (fast if ok else slow).append(it)
        res = {}
        self._keep = []
        for group, is_fast in ((fast, True), (slow, False)):
            if group:
                res.update(self._run_group(group, is_fast))
        return res

    def _run_group(self, items, is_fast):
        lib = L.lib()
        table = (L.WeightGradDesc * len(items))()
        res = {}
        dev = items[0].red.device
        for t, (p, red, want_w, want_b) in zip(table, items):
            g = p.plans[2]
            gm = p.ref.geom
            gw = torch.empty_like(p.ref.weight) if want_w else None
            gb = torch.empty_like(p.ref.bias) if (want_b and p.ref.bias is not None) else None
            t.dwpk, t.w_orig, t.grad = red.data_ptr(), p.ref.weight.data_ptr(), _ptr(gw)
            t.u_used, t.v_used, t.sigma = _ptr(p.u_used), _ptr(p.v_used), p.sigma.data_ptr()
            t.dbias_pk = red.data_ptr() + 4 * g.slab_elems
            t.grad_bias = _ptr(gb)
            t.Cout, t.Cin, t.KH, t.KW, t.shuffle2 = gm.cout, gm.cin, gm.k, gm.k, int(gm.shuffle2)
            t.CK, t.PS, t.KROWP, t.n_chunk, t.CoutPad = g.CK, g.PS, g.KROWP, g.n_chunk, g.CoutPad
            t.layout = int(p.kinds[2].bf16)
            res[id(p.ref)] = (gw, gb)
        tab = _table_to_device(table, dev)
        if is_fast:
            mco, mci = max(it.prep.ref.geom.cout for it in items), max(it.prep.ref.geom.cin for it in items)
            work = torch.empty((len(items) * ((mco + 31) // 32) * (mci // 32),), dtype=torch.float32, device=dev)
            L.check(lib.sisr_weights_grad_fast(tab.data_ptr(), len(items), work.data_ptr(), mco, mci, _stream()), 'sisr_weights_grad_fast')
        else:
            parts = max(L.check_count(lib.sisr_weights_grad_tiles(C.byref(t)), 'sisr_weights_grad_tiles') for t in table)
            work = torch.empty((parts * len(items),), dtype=torch.float32, device=dev)
            L.check(lib.sisr_weights_grad(tab.data_ptr(), len(items), work.data_ptr(), parts, _stream()), 'sisr_weights_grad')
        self._keep.append((tab, work))
        return res


class BackwardBook:
    """What the hand-scheduled backward passes of the generator and the discriminator keep alike: the weight gradients of their
    convs are collected (WgradDeepBatch: launched together; WeightGradBatch: un-packed together), the slab sums are deferred
    (PendingSlabs), and flush(tag) launches what is held back and announces every new gradient to the sink
    (distributed.GradReducer or None).  own_batch_slabs: the slab sums of the batched kernels wait in a list of their own
    (`batch_slabs`) instead of in `slabs`."""

    def __init__(self, P, refs, params, sink, own_batch_slabs):
        self.P, self.sink = P, sink
        self.grads = {}
        self.wg, self.wb = WeightGradBatch(), WgradDeepBatch()
        self.slabs = PendingSlabs()
        self.batch_slabs = PendingSlabs() if own_batch_slabs else self.slabs
        self.refs = {id(r): r for r in refs}
        self.by_id = {id(p): p for p in params}
        self.announced = set()

    def flush(self, tag):
        """un-pack the weight gradients collected so far (one launch) and announce every new gradient to the sink"""
        self.wb.run(self.batch_slabs)
        self.batch_slabs.flush()
        self.slabs.flush()                      # (nothing left, no launch, where the two are one list)
        grads = self.grads
        for ref_id, (gw, gb) in self.wg.run().items():
            ref = self.refs[ref_id]
            if gw is not None:
                grads[id(ref.weight)] = gw
            if gb is not None:
                grads[id(ref.bias)] = gb
        self.wg.items = []
        if self.sink is not None:
            new = [k for k in grads if k not in self.announced and k in self.by_id]
            self.announced.update(new)
            self.sink.ready([(self.by_id[k], grads[k]) for k in new], tag)

    def conv_bwd(self, ref, x_op, dy_op, need_dgrad=True, res=None, y_mode=L.Y_NHWC, bnb=None):
        """weight gradient (batched un-packing at the flush) + data gradient.  bnb = (x, consts, slope) names the BatchNorm (and
        the leaky activation behind it) the data gradient arrives at: where the conv kernel can, it emits that BatchNorm's
        backward reductions from its epilogue and (gradient, partial rows) is returned instead of the gradient."""
        p = self.P[id(ref)]
        want_w, want_b = ref.weight.requires_grad, ref.bias is not None and ref.bias.requires_grad
        if want_w or want_b:
            w = _wgrad_launch(p, x_op, dy_op)
            if self.wb.offer(w) is None:                # (the batch declines: that same record, in a launch of its own)
                _launch_wgrad(w, defer=self.slabs)
            self.wg.add(p, w.red, want_w, want_b)
        if not need_dgrad:
            return None
        if bnb is None:
            return conv_dgrad(p, dy_op, res=res, y_mode=y_mode)
        if can_fuse_bn_backward(p):
            return conv_dgrad(p, dy_op, res=res, y_mode=y_mode, bnb=bnb)
        return conv_dgrad(p, dy_op, res=res, y_mode=y_mode), None

    def toimage_bwd(self, ref, x_op, dy_op):
        """conv_bwd of the generator's last conv AND the slope gradient of the PReLU whose lazy activation x_op is, in one launch
        (toimage_backward) -> (data gradient, slope gradient), or None where that kernel does not take the layer"""
        p = self.P[id(ref)]
        want_w, want_b = ref.weight.requires_grad, ref.bias is not None and ref.bias.requires_grad
        if not (want_w or want_b):
            return None
        r = toimage_backward(p, x_op, dy_op, defer=self.slabs)
        if r is None:
            return None
        g, dslope, red = r
        self.wg.add(p, red, want_w, want_b)
        return g, dslope


class LazyBN:
    """BatchNorm constants [4, C] (scale, shift, batch mean, invstd) that are not computed yet: the statistics rows of
    the producing conv plus the module.  Where the conv that APPLIES this BatchNorm in its prologue runs on a persistent
    trunk kernel, that kernel finalises the statistics itself (SisrConvDesc.fin_*: one launch less per BatchNorm);
    anything else calls ensure(), which runs the stand-alone sisr_bn_finalize.  Either way `k` is valid in stream
    order after the consumer (or ensure()) has been launched."""
    __slots__ = ('sp', 'cp', 'bn', 'eps', 'momentum', 'k', 'done')

    def __init__(self, sp, cp, bn, eps=1e-5, momentum=0.1):
        self.sp, self.cp, self.bn, self.eps, self.momentum = sp, cp, bn, eps, momentum
        self.k = torch.empty((4, bn.weight.numel()), dtype=torch.float32, device=sp.device)
        self.done = False

    def ensure(self):
        if not self.done:
            bn_finalize(self.sp, self.cp, self.bn, self.eps, self.momentum, k=self.k)
            self.done = True
        return self.k

    def fill(self, d):
        """hand the finalisation to the conv of descriptor d"""
        bn = self.bn
        d.fin_stat, d.fin_cnt, d.fin_rows = self.sp.data_ptr(), self.cp.data_ptr(), self.sp.shape[0]
        d.fin_gamma, d.fin_beta = bn.weight.data_ptr(), bn.bias.data_ptr()
        d.fin_rm, d.fin_rv, d.fin_k = bn.running_mean.data_ptr(), bn.running_var.data_ptr(), self.k.data_ptr()
        d.fin_momentum, d.fin_eps = self.momentum, self.eps


def bn_finalize(sp, cp, bn, eps=1e-5, momentum=0.1, k=None):
    """-> consts [4, C]: scale, shift, batch mean, invstd (written into `k` when given); updates bn.running_* in place."""
    lib = L.lib()
    cch = bn.weight.numel()
    if k is None:
        k = torch.empty((4, cch), dtype=torch.float32, device=sp.device)
    L.check(lib.sisr_bn_finalize(sp.data_ptr(), cp.data_ptr(), sp.shape[0], cch, bn.weight.data_ptr(),
                                 bn.bias.data_ptr(), bn.running_mean.data_ptr(), bn.running_var.data_ptr(),
                                 momentum, eps, k[0].data_ptr(), k[1].data_ptr(), k[2].data_ptr(),
                                 k[3].data_ptr(), _stream()), 'sisr_bn_finalize')
    return k


def bn_eval_consts(bn, eps=1e-5):
    lib = L.lib()
    cch = bn.weight.numel()
    k = torch.empty((4, cch), dtype=torch.float32, device=bn.weight.device)
    L.check(lib.sisr_bn_eval_consts(bn.weight.data_ptr(), bn.bias.data_ptr(), bn.running_mean.data_ptr(),
                                    bn.running_var.data_ptr(), eps, cch, k[0].data_ptr(), k[1].data_ptr(),
                                    _stream()), 'sisr_bn_eval_consts')
    return k


def bn_backward(dy, x, consts, gamma, slope=None, part=None, slabs=None):
    """Reductions of BatchNorm backward (+ the leaky activation after it when slope is given).
    Returns (q [3,C] = qa,qb,qd ; dgamma ; dbeta ; dslope or None).  part: per-tile partial rows already written
    by the conv that produced dy (conv_dgrad(..., bnb=...)); only the finishing kernel runs then -- and, given `slabs`
    (PendingSlabs), that launch also carries one deferred slab reduction."""
    lib = L.lib()
    cch = x.shape[-1]
    d = L.BnBwdDesc()
    d.P, d.C = x.numel() // cch, cch
    d.act_mode = 0 if slope is None else 1
    d.slope_p, d.slope = _slope(slope)
    dev = x.device
    if part is None:
        L.check(lib.sisr_bn_bwd_plan(C.byref(d)), 'sisr_bn_bwd_plan')
        work = torch.empty((d.grid, 2 * cch + 1), dtype=torch.float32, device=dev)
    else:
        work, d.grid = part, part.shape[0]
    q = torch.empty((3, cch), dtype=torch.float32, device=dev)
    dgamma = torch.empty((cch,), dtype=torch.float32, device=dev)
    dbeta = torch.empty((cch,), dtype=torch.float32, device=dev)
    dslope = torch.empty((1,), dtype=torch.float32, device=dev) if slope is not None else None
    d.dy, d.x = dy.data_ptr(), x.data_ptr()
    d.dy_bf16, d.x_bf16 = _bf(dy), _bf(x)
    d.scale, d.shift, d.mean, d.invstd = (consts[0].data_ptr(), consts[1].data_ptr(), consts[2].data_ptr(),
                                          consts[3].data_ptr())
    d.gamma, d.work = gamma.data_ptr(), work.data_ptr()
    d.qa, d.qb, d.qd = q[0].data_ptr(), q[1].data_ptr(), q[2].data_ptr()
    d.dgamma, d.dbeta, d.dslope = dgamma.data_ptr(), dbeta.data_ptr(), _ptr(dslope)
    if part is None:
        L.check(lib.sisr_bn_bwd(C.byref(d), _stream()), 'sisr_bn_bwd')
    else:
        job = slabs.pop() if slabs is not None else None
        if job is not None:                     # this launch also sums the slabs of the weight gradient computed before it
            L.check(lib.sisr_bn_bwd_finalize_slab(C.byref(d), job.slab.data_ptr(), job.red.data_ptr(), job.n_slabs, job.stride, job.lead,
                                                  _stream()), 'sisr_bn_bwd_finalize_slab')
        else:
            L.check(lib.sisr_bn_bwd_finalize(C.byref(d), _stream()), 'sisr_bn_bwd_finalize')
    return q, dgamma, dbeta, dslope


def eltwise_res_affine(x1, slope1, x2=None, pa=None, pd=None):
    """y = lrelu(x1, slope1) + (pa*x2 + pd | x2 | 0) over NHWC tensors."""
    lib = L.lib()
    cch = x1.shape[-1]
    y = torch.empty(x1.shape, dtype=act_dtype(cch), device=x1.device)
    sp, sv = _slope(slope1)
    dt = _bf(x1) | (_bf(x2) << 1) | (_bf(y) << 2)
    L.check(lib.sisr_eltwise_res_affine(x1.data_ptr(), sp, sv, _ptr(x2), _ptr(pa), _ptr(pd), y.data_ptr(),
                                        x1.numel() // cch, cch, dt, _stream()), 'sisr_eltwise_res_affine')
    return y


def prelu_slope_grad(dy, pre):
    lib = L.lib()
    work = torch.empty((1024,), dtype=torch.float32, device=dy.device)
    out = torch.empty((1,), dtype=torch.float32, device=dy.device)
    L.check(lib.sisr_prelu_slope_grad(dy.data_ptr(), pre.data_ptr(), dy.numel(), work.data_ptr(),
                                      out.data_ptr(), _bf(dy) | (_bf(pre) << 1), _stream()), 'sisr_prelu_slope_grad')
    return out


def add(a, b):
    lib = L.lib()
    if a.dtype != b.dtype:
        raise RuntimeError('add: operands with mixed storage types')
    y = torch.empty_like(a)
    L.check(lib.sisr_add(a.data_ptr(), b.data_ptr(), y.data_ptr(), a.numel(), 7 * _bf(a), _stream()), 'sisr_add')
    return y


def require_gpu_tensor(x, what):
    if not (isinstance(x, torch.Tensor) and x.is_cuda):
        raise RuntimeError('%s: this path runs only on an MI355X device tensor (got %s); there is no '
                           'CPU fallback' % (what, getattr(x, 'device', type(x))))
    if x.dtype != torch.float32:
        raise RuntimeError('%s: fp32 tensors expected at the module boundary, got %s' % (what, x.dtype))


def nhwc_to_nchw(x, out, dst_stride, pa=None, pd=None, slope=None):
    """materialise lrelu(pa*x+pd, slope) from NHWC x into an NCHW destination (rows of `out`)."""
    n, h, w, c = x.shape
    sp, sv = _slope(slope)
    L.check(L.lib().sisr_nhwc_to_nchw(x.data_ptr(), _ptr(pa), _ptr(pd), sp, sv, out.data_ptr(), dst_stride,
                                      n, h, w, c, _bf(x), _stream()), 'sisr_nhwc_to_nchw')


def nchw_to_nhwc(src, src_stride, n, h, w, c):
    y = torch.empty((n, h, w, c), dtype=act_dtype(c), device=src.device)
    L.check(L.lib().sisr_nchw_to_nhwc(src.data_ptr(), src_stride, y.data_ptr(), n, h, w, c, _bf(y), _stream()),
            'sisr_nchw_to_nhwc')
    return y


FC_MAX_BATCH = 16          # rows the FC kernels keep in registers (FC_B in layout_fc.hip); larger batches run in slices


def fc_forward(x, w, b, in_slope=1.0, sigmoid=False):
    bsz, k = x.shape
    y = torch.empty((bsz, w.shape[0]), dtype=torch.float32, device=x.device)
    for b0 in range(0, bsz, FC_MAX_BATCH):
        nb = min(FC_MAX_BATCH, bsz - b0)
        L.check(L.lib().sisr_fc_forward(x[b0:b0 + nb].data_ptr(), in_slope, w.data_ptr(), _ptr(b), y[b0:b0 + nb].data_ptr(),
                                        nb, k, w.shape[0], int(sigmoid), _stream()), 'sisr_fc_forward')
    return y


def fc_backward(dy, x, w, in_slope=1.0, need_dx=True):
    """-> (dx wrt lrelu(x) [B,K] or None, dW, db)"""
    lib = L.lib()
    bsz, k = x.shape
    nout = w.shape[0]
    dw = db = None
    dx = torch.empty((bsz, k), dtype=torch.float32, device=x.device) if need_dx else None
    for b0 in range(0, bsz, FC_MAX_BATCH):
        nb = min(FC_MAX_BATCH, bsz - b0)
        dyc, xc = dy[b0:b0 + nb], x[b0:b0 + nb]
        dwc = torch.empty_like(w)
        dbc = torch.empty((nout,), dtype=torch.float32, device=x.device)
        L.check(lib.sisr_fc_wgrad(dyc.data_ptr(), xc.data_ptr(), in_slope, dwc.data_ptr(), dbc.data_ptr(), nb, k, nout,
                                  _stream()), 'sisr_fc_wgrad')
        dw, db = (dwc, dbc) if dw is None else (add(dw, dwc), add(db, dbc))     # batch slices sum into the gradient
        if need_dx:
            splits = lib.sisr_fc_dgrad_splits(k, nout)
            work = torch.empty((splits, nb, k), dtype=torch.float32, device=x.device)
            L.check(lib.sisr_fc_dgrad(dyc.data_ptr(), w.data_ptr(), dx[b0:b0 + nb].data_ptr(), work.data_ptr(), nb, k, nout,
                                      _stream()), 'sisr_fc_dgrad')
    return dx, dw, db


def fc_head_ok(bsz, k, n):
    """the classifier head of D runs on fc_head.hip (exact-fp32 MFMA weight streaming): 1 to 16 batch rows, K in 64s, N in 128s
    (what sisr_fc1_dgrad takes; the forward alone takes K and N in 16s, the backward any N).  Empty shapes are refused there too."""
    return 0 < bsz <= FC_MAX_BATCH and k > 0 and k % 64 == 0 and n > 0 and n % 128 == 0


def fc_head_forward(x, w1, b1, w2, b2, slope):
    """-> (h1 [B, N] pre-activation, y [B, 1]) of Linear -> LeakyReLU -> Linear(N, 1) -> Sigmoid"""
    lib = L.lib()
    bsz, k = x.shape
    n = w1.shape[0]
    h1 = torch.empty((bsz, n), dtype=torch.float32, device=x.device)
    y = torch.empty((bsz, 1), dtype=torch.float32, device=x.device)
    ws = torch.empty((lib.sisr_fc_head_ws_floats(n),), dtype=torch.float32, device=x.device)
    L.check(lib.sisr_fc_head_forward(x.data_ptr(), w1.data_ptr(), _ptr(b1), w2.data_ptr(), _ptr(b2), slope, h1.data_ptr(),
                                     y.data_ptr(), ws.data_ptr(), bsz, k, n, _stream()), 'sisr_fc_head_forward')
    return h1, y


def fc_head_backward(g, y, h1, w2, slope):
    """-> (d1 [B, N], dW2 like w2, db2 [1], db1 [N])"""
    lib = L.lib()
    bsz, n = h1.shape
    dev = h1.device
    d1 = torch.empty_like(h1)
    dw2 = torch.empty_like(w2)
    db2 = torch.empty((1,), dtype=torch.float32, device=dev)
    db1 = torch.empty((n,), dtype=torch.float32, device=dev)
    L.check(lib.sisr_fc_head_backward(g.data_ptr(), y.data_ptr(), h1.data_ptr(), w2.data_ptr(), slope, d1.data_ptr(),
                                      dw2.data_ptr(), db2.data_ptr(), db1.data_ptr(), bsz, n, _stream()), 'sisr_fc_head_backward')
    return d1, dw2, db2, db1


def fc1_dgrad(d1, w1):
    bsz, n = d1.shape
    k = w1.shape[1]
    dx = torch.empty((bsz, k), dtype=torch.float32, device=d1.device)
    L.check(L.lib().sisr_fc1_dgrad(d1.data_ptr(), w1.data_ptr(), dx.data_ptr(), bsz, k, n, _stream()), 'sisr_fc1_dgrad')
    return dx


def fc_wgrad_rows_ok(rows, k, n):
    """sisr_fc_wgrad_rows takes the gathered factors of `rows` batch rows (all ranks)"""
    return 0 < rows <= 256 and k > 0 and k % 128 == 0 and n > 0 and n % 64 == 0


def fc_wgrad_rows(dy_all, x_all, w, scale):
    """dW = scale * dy_all^T x_all over the rows of ALL ranks (the gathered factors of the classifier head's weight gradient)"""
    rows, k = x_all.shape
    dw = torch.empty_like(w)
    L.check(L.lib().sisr_fc_wgrad_rows(dy_all.data_ptr(), x_all.data_ptr(), float(scale), dw.data_ptr(), rows, k, w.shape[0], _stream()),
            'sisr_fc_wgrad_rows')
    _count('fc_wgrad_rows')
    return dw


def fc_wgrad_only(dy, x, w, in_slope=1.0):
    """dW = dy^T lrelu(x) (no bias gradient, no data gradient)"""
    bsz, k = x.shape
    dw = torch.empty_like(w)
    L.check(L.lib().sisr_fc_wgrad(dy.data_ptr(), x.data_ptr(), in_slope, dw.data_ptr(), None, bsz, k, w.shape[0], _stream()),
            'sisr_fc_wgrad')
    return dw


def act_bwd(dy, ref, kind, slope=0.0):
    out = torch.empty_like(dy)
    L.check(L.lib().sisr_act_bwd(dy.data_ptr(), ref.data_ptr(), out.data_ptr(), dy.numel(), kind, slope,
                                 _stream()), 'sisr_act_bwd')
    return out


def maxpool2(x):
    n, h, w, c = x.shape
    y = torch.empty((n, h // 2, w // 2, c), dtype=x.dtype, device=x.device)
    L.check(L.lib().sisr_maxpool2_fwd(x.data_ptr(), y.data_ptr(), n, h, w, c, 3 * _bf(x), _stream()), 'sisr_maxpool2_fwd')
    return y


def maxpool2_relu_bwd(dy, x):
    n, h, w, c = x.shape
    if dy.dtype != x.dtype:
        raise RuntimeError('maxpool2_relu_bwd: gradient and activation with mixed storage types')
    dx = torch.empty_like(x)
    L.check(L.lib().sisr_maxpool2_relu_bwd(dy.data_ptr(), x.data_ptr(), dx.data_ptr(), n, h, w, c, 7 * _bf(x), _stream()),
            'sisr_maxpool2_relu_bwd')
    return dx


def add_relu_masked(a, b, ref):
    out = torch.empty_like(b)
    dt = _bf(a) | (_bf(b) << 1) | (_bf(ref) << 2) | (_bf(out) << 3)
    L.check(L.lib().sisr_add_relu_masked(_ptr(a), b.data_ptr(), ref.data_ptr(), out.data_ptr(), b.numel(), dt,
                                         _stream()), 'sisr_add_relu_masked')
    return out
