"""A differentiable fp32 image resize with torch's half-pixel coordinates on the device, the mode chosen per sample
(csrc/resize.hip).

``resize(x, size, mode)`` is ``F.interpolate(x, size, mode=mode, align_corners=False)`` for 'bilinear' and 'bicubic' (no
antialias) and ``F.interpolate(x, size, mode='area')``, up or down, any ratio -- with ONE difference: ``mode`` may also be an
int32 device tensor [N] (0 area, 1 bilinear, 2 bicubic) that gives every sample of the batch its own resampler.  The kernel
reads the table, the host never does, so a captured call follows whatever the table holds at replay.  One launch forward and one
backward (the exact transpose, gathered: no atomics, the same bits on every call); nothing but the table is kept for the backward
pass, the operator is linear.

>>> y = resize(x, (136, 136), 'area')
>>> modes = torch.tensor([2, 0, 1], dtype=torch.int32, device='cuda')
>>> y = resize(x, (136, 136), modes)                      # sample 0 bicubic, 1 area, 2 bilinear

``resize_taps`` returns the 1-D operator as a dense matrix and ``expected_resize_modes`` restates the random mode draw of
``degrade.HighOrderDegrader(resize_probs=...)``; both are host code and need no GPU.  No CPU path: CPU tensors are refused.
"""
import ctypes as C
import sys
import types

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _lib as L
from .draws import step_tensor
from .engine import _stream, require_gpu_tensor

MODES = ('area', 'bilinear', 'bicubic')          # the index is the code of the device table
_TABLES = {}                                     # (code, N, device) -> the constant table of a mode given by name


def _mode_code(mode, who):
    if mode not in MODES:
        raise ValueError("%s: mode is 'area', 'bilinear' or 'bicubic' (or an int32 device tensor [N]), got %r" % (who, mode))
    return MODES.index(mode)


def resize_taps(mode, in_size, out_size):
    """The 1-D operator of ``mode`` for ``in_size`` -> ``out_size`` as a dense float64 numpy matrix [out_size, in_size], built from
    the library's host table (sisr_resize_taps_host: the kernels' own text compiled for the host): the fp32 weights, the indices
    clamped to the axis, taps that meet on a border pixel added.  ``resize`` computes ``R_h x R_w^T``."""
    code, n_in, n_out = _mode_code(mode, 'resize_taps'), int(in_size), int(out_size)
    if n_in < 1 or n_out < 1:
        raise ValueError('resize_taps: the sizes must be >= 1, got %d -> %d' % (n_in, n_out))
    first, count = np.zeros(n_out, np.int32), np.zeros(n_out, np.int32)
    w = np.zeros((n_out, L.RESIZE_MAX_TAPS), np.float32)
    L.check(L.lib().sisr_resize_taps_host(code, n_in, n_out, first.ctypes.data_as(C.c_void_p), count.ctypes.data_as(C.c_void_p),
                                          w.ctypes.data_as(C.c_void_p)), 'sisr_resize_taps_host')
    R = np.zeros((n_out, n_in), np.float64)
    for o in range(n_out):
        for k in range(int(count[o])):
            R[o, min(max(int(first[o]) + k, 0), n_in - 1)] += float(w[o, k])
    return R


def _check_probs(probs, who):
    p = tuple(float(v) for v in probs)
    if len(p) != 3 or not all(np.isfinite(v) and v >= 0.0 for v in p) or not sum(p) > 0.0:
        raise ValueError('%s: three finite weights >= 0 with a positive sum (area, bilinear, bicubic) are expected, got %r' % (who, probs))
    return p


def expected_resize_modes(seed, t, B, probs, rank=0):
    """Host, no GPU (sisr_resize_modes_host: the device code's own text compiled for the host): the modes that
    ``HighOrderDegrader(resize_probs=probs)`` draws for a batch of ``B`` on the drawn step ``t`` -> int32 numpy array [B]."""
    B, p = int(B), _check_probs(probs, 'expected_resize_modes')
    if B < 1 or int(t) < 0:
        raise ValueError('expected_resize_modes: B must be >= 1 and t >= 0, got %d, %d' % (B, int(t)))
    m = np.zeros(B, np.int32)
    L.check(L.lib().sisr_resize_modes_host(int(t), int(seed), int(rank), B, p[0], p[1], p[2], m.ctypes.data_as(C.c_void_p)),
            'sisr_resize_modes_host')
    return m


def draw_resize_modes(drawn_step, seed, rank, B, probs):
    """One launch (sisr_resize_modes_draw): the modes of a batch of ``B`` on the step held by ``drawn_step`` (a 0-dim int64 device
    tensor, read and NOT advanced) -> int32 device tensor [B]"""
    p = _check_probs(probs, 'draw_resize_modes')
    step_tensor(drawn_step, strict='draw_resize_modes')
    modes = torch.empty(int(B), dtype=torch.int32, device=drawn_step.device)
    L.check(L.lib().sisr_resize_modes_draw(drawn_step.data_ptr(), int(seed), int(rank), int(B), p[0], p[1], p[2], modes.data_ptr(),
                                           _stream()), 'sisr_resize_modes_draw')
    return modes


class _Resize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, size, modes):
        x = x.detach()
        n, c, h, w = x.shape
        y = torch.empty((n, c, size[0], size[1]), dtype=torch.float32, device=x.device)
        L.check(L.lib().sisr_resize_fwd(x.data_ptr(), modes.data_ptr(), y.data_ptr(), n, c, h, w, size[0], size[1], _stream()),
                'sisr_resize_fwd')
        ctx.shape = (n, c, h, w, size[0], size[1])
        ctx.save_for_backward(modes)               # nothing else: the operator is linear
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        n, c, h, w, oh, ow = ctx.shape
        modes, = ctx.saved_tensors
        g = g.to(torch.float32).contiguous()
        dx = torch.empty((n, c, h, w), dtype=torch.float32, device=g.device)
        L.check(L.lib().sisr_resize_bwd(g.data_ptr(), modes.data_ptr(), dx.data_ptr(), n, c, h, w, oh, ow, _stream()), 'sisr_resize_bwd')
        return dx, None, None


def resize(x, size, mode='bicubic'):
    """x [N, C, H, W] fp32 on the device -> [N, C, size[0], size[1]], torch's ``F.interpolate`` with ``align_corners=False`` (see
    the module text).  ``mode``: 'area', 'bilinear' or 'bicubic' for every sample (a device table per (mode, N) is made on first use
    and kept), or an int32 device tensor [N] of codes 0 / 1 / 2 that is used as given and kept for the backward pass; a code outside
    0 .. 2 resamples bicubically.  Differentiable with respect to ``x``, once; deterministic."""
    if not isinstance(x, torch.Tensor):                         # argument errors first, whatever the tensor lives on; then the device
        raise RuntimeError('resize input: a device tensor is expected, got %s' % type(x))
    if x.dim() != 4 or x.dtype != torch.float32:
        raise ValueError('resize: an fp32 [N, C, H, W] batch is expected, got %s %s' % (x.dtype, tuple(x.shape)))
    size = (int(size[0]), int(size[1]))
    if min(size) < 1:
        raise ValueError('resize: the output size must be >= 1, got %s' % (size,))
    require_gpu_tensor(x, 'resize input')
    n = int(x.shape[0])
    if isinstance(mode, torch.Tensor):
        if mode.dtype != torch.int32 or tuple(mode.shape) != (n,) or not mode.is_contiguous():
            raise ValueError('resize: a mode table must be a contiguous int32 tensor [N = %d], got %s %s' % (n, mode.dtype, tuple(mode.shape)))
        if mode.device != x.device:
            raise RuntimeError('resize: the batch is on %s, the mode table on %s' % (x.device, mode.device))
        modes = mode
    else:
        key = (_mode_code(mode, 'resize'), n, x.device)
        modes = _TABLES.get(key)
        if modes is None:
            modes = _TABLES[key] = torch.full((n,), key[0], dtype=torch.int32, device=x.device)
    return _Resize.apply(x.contiguous(), size, modes)


class _CallableModule(types.ModuleType):
    """The import system binds the package attribute ``resize`` to this MODULE as soon as it is imported, whatever the package's lazy
    names say; calling the module is calling ``resize``, so ``sisr.resize(x, size, mode)`` works in either order of imports."""

    def __call__(self, *args, **kwargs):
        return resize(*args, **kwargs)


sys.modules[__name__].__class__ = _CallableModule
