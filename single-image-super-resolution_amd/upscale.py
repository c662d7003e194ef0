"""Whole-image super-resolution: image in, image x s out.

Every forward entry point of the package takes a fixed-size batch of patches; ``Upscaler`` applies a trained generator to an image
of ANY size by cutting it into overlapping tiles of one shape, running the generator over them as ordinary batches in eval mode
and stitching the SR tiles on the device (csrc/tiles.hip):

>>> up = Upscaler(net_g)                      # tile 192, halo = receptive_halo(net_g): the whole-image forward, not an approximation
>>> sr_u8 = up(image_u8)                      # [H, W, C] uint8 on the device -> [s H, s W, C] uint8
>>> sr = up(image_f32)                        # [C, H, W] fp32, normalised     -> [C, s H, s W] fp32

With ``halo >= receptive_halo(net_g)`` every output pixel is computed from exactly the LR pixels the whole-image forward reads
(a window that reaches an image border is flush with it, so the convolutions' zero padding coincides with the real border): the
result IS the whole-image forward, at (tile / (tile - 2 halo))^2 times its arithmetic -- 2.9x at the defaults (tile 192, halo 40),
1.9x at tile 288.  A smaller halo is the user's speed / seam trade; ``feather`` cross-fades the seams for that case, and
``ensemble=8`` averages the eight flips / transpositions of the input (the geometric self-ensemble of Lim et al., EDSR, CVPRW 2017).

Everything runs on the current stream; nothing reads back to the host.  The planner (``TilePlan``, ``tile_axis``), the weight
formula (``axis_weights``) and ``receptive_halo`` are host code and need no GPU.
"""
import contextlib
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from .engine import _stream
from .metrics import niqe, psnr_ssim
from .utils import lr_from_hr


def receptive_halo(net_g):
    """LR pixels on each side that one output pixel of ``net_g`` (any member of the generator family) depends on, from its
    ``Topology``: r = 4 behind the end conv (0 without one), r = ceil(r / 2) + 1 through every upscale stage backwards (a 3 x 3
    conv in front of a PixelShuffle(2)), then 1 for the trunk's end conv, 2 per residual block and 4 for the first 9 x 9 conv.
    An upper bound by one or two pixels where the end conv is 3 x 3; the standard 16-block x2 / x4 / x8 nets all give 40."""
    topo = net_g._topology()
    r = 4 if topo.end is not None else 0
    for _ in topo.stages:
        r = -(-r // 2) + 1
    return r + 1 + 2 * len(topo.blocks) + 4


def tile_axis(L_, T, halo):
    """sisr_tile_axis (host code of the library): the plan of one axis -> (a, b) int32 arrays of n origins and n ownership
    boundaries; window i is [a_i, a_i + min(T, L)) and owns [b_{i-1}, b_i), b_{-1} = 0.  ValueError for what the library refuses."""
    L_, T, halo = int(L_), int(T), int(halo)
    lib = L.lib()
    n = lib.sisr_tile_axis(L_, T, halo, None, None, 0)
    if n < 1:
        raise ValueError('tile_axis: extent %d, tile %d, halo %d: sizes must be >= 1, halo >= 0 and, for an image larger than the '
                         'tile, tile - 2 halo >= 1' % (L_, T, halo))
    a, b = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    L.check_count(lib.sisr_tile_axis(L_, T, halo, a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), n), 'sisr_tile_axis')
    return a, b


def axis_weights(b, scale, feather, extent):
    """Pure numpy (fp64): the normalised per-axis stitch weights of sisr_tile_stitch -> [n, scale * extent], column Y the weights of
    output position Y (LR position p = (Y + 0.5) / scale) over the n tiles whose ownership boundaries are ``b``.  For audits and
    tests: every column sums to 1."""
    b = np.asarray(b, dtype=np.float64)
    n, f = b.shape[0], float(feather)
    p = (np.arange(int(scale) * int(extent), dtype=np.float64) + 0.5) / float(scale)
    lo = np.concatenate([[0.0], b[:-1]])[:, None]                       # b_{i-1}
    hi = b[:, None]
    if f == 0.0:
        r = ((p >= lo) & (p < hi)).astype(np.float64)
    else:
        dl = (p - (lo - f)) / (2.0 * f)
        dr = ((hi + f) - p) / (2.0 * f)
        dl[0], dr[n - 1] = np.inf, np.inf
        r = np.clip(np.minimum(dl, dr), 0.0, 1.0)
    return r / r.sum(axis=0, keepdims=True)


class TilePlan:
    """The tiles of an H x W image: the outer product of two axis plans, numbered row-major, all of shape
    (th, tw) = (min(tile, H), min(tile, W)).  ``ay, by, ax, bx``: the axis plans; ``table``: [n, 4] int32 rows (0, y0, x0, 0)."""

    def __init__(self, H, W, tile, halo):
        self.H, self.W, self.tile, self.halo = int(H), int(W), int(tile), int(halo)
        self.ay, self.by = tile_axis(self.H, self.tile, self.halo)
        self.ax, self.bx = tile_axis(self.W, self.tile, self.halo)
        self.ny, self.nx = len(self.ay), len(self.ax)
        self.n = self.ny * self.nx
        self.th, self.tw = min(self.tile, self.H), min(self.tile, self.W)
        self.table = np.zeros((self.n, 4), dtype=np.int32)
        self.table[:, 1] = np.repeat(self.ay, self.nx)
        self.table[:, 2] = np.tile(self.ax, self.ny)

    def ensemble_table(self, E):
        """[E n, 4]: member e's tiles at rows e n ... e n + n - 1 with ops e"""
        t = np.tile(self.table, (E, 1))
        t[:, 3] = np.repeat(np.arange(E, dtype=np.int32), self.n)
        return t


class _DevicePlan:
    """a TilePlan with its table and axis arrays on the device"""

    def __init__(self, plan, E, dev):
        self.plan = plan
        self.table = torch.from_numpy(plan.ensemble_table(E)).to(dev)
        self.ay, self.by, self.ax, self.bx = (torch.from_numpy(v).to(dev) for v in (plan.ay, plan.by, plan.ax, plan.bx))


class Upscaler:
    """``up(image)``: the generator over the whole image, tiled (module docstring).

    ``tile``      LR pixels per tile side.  ``halo``: LR pixels of context on every interior tile side; None: ``receptive_halo(net_g)``.
    ``feather``   0 <= feather <= halo: half-width (LR pixels) of the linear cross-fade around every ownership boundary; 0: none.
                  A cross-fade blends pixels up to ``feather`` beyond the boundary, so it keeps the result exact only where
                  halo >= receptive_halo + feather; it is meant for the smaller halos, whose seams it softens.
    ``ensemble``  1, or 8: the mean over the eight flips / transpositions (square tiles only).
    ``batch``     tiles per generator call.  ``ema``: an ``ema.WeightEMA`` over ``net_g``; the forward runs inside ``ema.applied()``.
    ``mean, std`` the normalisation of uint8 images (ToTensor + Normalize, as the patch sources).

    The generator runs in eval mode under ``no_grad`` exactly as ``metrics.evaluate_generator`` runs it: every buffer of ``net_g`` is
    bit-unchanged afterwards and every module's training flag is restored, also when the forward raises.  Per call: the plan (cached
    per image size, with its device tables), one gather launch, the generator over slices of ``batch`` tiles, one stitch launch."""

    def __init__(self, net_g, tile=192, halo=None, feather=0, ensemble=1, batch=8, ema=None, mean=0.5, std=0.5):
        self.net_g, self.ema = net_g, ema
        self.tile, self.batch, self.ensemble = int(tile), int(batch), int(ensemble)
        self.halo = receptive_halo(net_g) if halo is None else int(halo)
        self.feather, self.mean, self.std = float(feather), float(mean), float(std)
        if ema is not None and ema.module is not net_g:
            raise ValueError('Upscaler: ema averages another module than net_g')
        if self.tile < 1 or self.batch < 1 or self.halo < 0:
            raise ValueError('Upscaler: tile and batch must be >= 1 and halo >= 0, got tile %d, batch %d, halo %d'
                             % (self.tile, self.batch, self.halo))
        if self.ensemble not in (1, 8):
            raise ValueError('Upscaler: ensemble must be 1 or 8, got %d' % self.ensemble)
        if not 0.0 <= self.feather <= self.halo:
            raise ValueError('Upscaler: feather must lie in [0, halo = %d], got %r' % (self.halo, feather))
        if self.std == 0.0:
            raise ValueError('Upscaler: std must not be 0')
        self.scale = 2 ** len(net_g._topology().stages)
        if self.scale > 8:
            raise ValueError('Upscaler: scale factors up to 8 are supported, the generator has %d' % self.scale)
        self._plans = {}

    # ---- planning ---------------------------------------------------------------------------------------------------------------
    def plan(self, H, W):
        """the TilePlan of an H x W image (host only); ValueError where the settings cannot tile it"""
        H, W = int(H), int(W)
        if H < 1 or W < 1:
            raise ValueError('Upscaler: the image is %d x %d' % (H, W))
        if max(H, W) > self.tile and self.tile - 2 * self.halo < 1:
            raise ValueError('Upscaler: a %d x %d image needs tiles, and tile %d leaves no core around a halo of %d on each side; '
                             'use tile >= %d' % (H, W, self.tile, self.halo, 2 * self.halo + 1))
        plan = TilePlan(H, W, self.tile, self.halo)
        if self.ensemble == 8 and plan.th != plan.tw:
            side = min(H, W)
            fits = 'tile=%d' % side if side - 2 * self.halo >= 1 else 'tile=%d with halo <= %d' % (side, (side - 1) // 2)
            raise ValueError('Upscaler: ensemble=8 transposes tiles and needs square ones; a %d x %d image gives %d x %d tiles with '
                             'tile=%d -- %s would work' % (H, W, plan.th, plan.tw, self.tile, fits))
        return plan

    def _device_plan(self, H, W, dev):
        key = (H, W, str(dev))
        if key not in self._plans:
            self._plans[key] = _DevicePlan(self.plan(H, W), self.ensemble, dev)
        return self._plans[key]

    # ---- the call ---------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _kind(image):
        if isinstance(image, torch.Tensor) and image.dim() == 3:
            if image.dtype == torch.uint8 and 1 <= image.shape[2] <= 4:
                return 'u8'
            if image.dtype == torch.float32 and 1 <= image.shape[0] <= 4:
                return 'f32'
        raise RuntimeError('Upscaler: a [H, W, C] uint8 image or a [C, H, W] fp32 image (1 to 4 channels) on the MI355X is expected, '
                           'got %s %s' % (getattr(image, 'dtype', type(image)), tuple(getattr(image, 'shape', ()))))

    def __call__(self, image):
        """[H, W, C] uint8 -> [s H, s W, C] uint8; [C, H, W] fp32 (normalised) -> [C, s H, s W] fp32"""
        return self._run(image, self._kind(image) == 'u8')

    def to_float(self, image_u8):
        """the fp32 result [C, s H, s W] (normalised units) for a [H, W, C] uint8 input"""
        if self._kind(image_u8) != 'u8':
            raise RuntimeError('Upscaler.to_float: a [H, W, C] uint8 image is expected, got %s' % image_u8.dtype)
        return self._run(image_u8, False)

    def _run(self, image, u8_out):
        kind = self._kind(image)
        if not image.is_cuda:
            raise RuntimeError('Upscaler: this path runs only on an MI355X device tensor (got one on %s); there is no CPU fallback'
                               % image.device)
        image = image.contiguous()
        (H, W, Cimg) = image.shape if kind == 'u8' else (image.shape[1], image.shape[2], image.shape[0])
        dp = self._device_plan(int(H), int(W), image.device)
        p, lib, s, E = dp.plan, L.lib(), self.scale, self.ensemble
        rows = E * p.n
        tiles = torch.empty((rows, Cimg, p.th, p.tw), dtype=torch.float32, device=image.device)
        if kind == 'u8':
            L.check(lib.sisr_patch_gather(image.data_ptr(), 1, H, W, Cimg, dp.table.data_ptr(), rows, p.th, p.tw, self.mean, self.std,
                                          tiles.data_ptr(), 0, _stream()), 'sisr_patch_gather')
        else:
            L.check(lib.sisr_tile_gather_f32(image.data_ptr(), Cimg, H, W, dp.table.data_ptr(), rows, p.th, p.tw, tiles.data_ptr(),
                                             _stream()), 'sisr_tile_gather_f32')
        sr = torch.empty((rows, Cimg, s * p.th, s * p.tw), dtype=torch.float32, device=image.device)
        net_g = self.net_g
        modes = [(m, m.training) for m in net_g.modules()]
        with contextlib.nullcontext() if self.ema is None else self.ema.applied():
            try:
                net_g.eval()
                with torch.no_grad():
                    for i in range(0, rows, self.batch):
                        out = net_g(tiles[i:i + self.batch])
                        if out.shape[1:] != sr.shape[1:]:
                            raise ValueError('Upscaler: the generator maps %s tiles to %s, %s was expected'
                                             % (tuple(tiles.shape[1:]), tuple(out.shape[1:]), tuple(sr.shape[1:])))
                        sr[i:i + self.batch].copy_(out)
            finally:
                for m, was in modes:
                    m.training = was
        if u8_out:
            dst = torch.empty((s * H, s * W, Cimg), dtype=torch.uint8, device=image.device)
        else:
            dst = torch.empty((Cimg, s * H, s * W), dtype=torch.float32, device=image.device)
        self.stitch(sr, dp, dst)
        return dst

    def stitch(self, sr_tiles, dp, dst):
        """the one stitch launch: ``sr_tiles`` [E n, C, s th, s tw] fp32 -> ``dst`` ([C, s H, s W] fp32 or [s H, s W, C] uint8)"""
        p = dp.plan
        L.check(L.lib().sisr_tile_stitch(sr_tiles.data_ptr(), dp.table.data_ptr(), dp.ay.data_ptr(), dp.by.data_ptr(), p.ny,
                                         dp.ax.data_ptr(), dp.bx.data_ptr(), p.nx, sr_tiles.shape[1], p.H, p.W, p.th, p.tw,
                                         self.scale, self.halo, self.feather, self.ensemble, self.mean, self.std, dst.data_ptr(),
                                         int(dst.dtype == torch.uint8), _stream()), 'sisr_tile_stitch')
        return dst


def evaluate_image(up, img_hr_u8, image_size_lr=None, niqe_model=None):
    """One whole-image validation: the [H, W, C] uint8 HR image is normalised, degraded with ``lr_from_hr`` to ``image_size_lr``
    (None: (H // s, W // s)), upscaled tiled by ``up`` and scored against the HR image with ``psnr_ssim`` (borders cropped by the
    scale factor, the SR convention) -> ``dict(psnr=Tensor[1], ssim=Tensor[1])``.  H and W must be s times the LR size.
    ``niqe_model`` (a ``metrics.NiqeModel``): the dict gains ``niqe``, the no-reference score of the SR image, cropped alike."""
    if Upscaler._kind(img_hr_u8) != 'u8':
        raise RuntimeError('evaluate_image: a [H, W, C] uint8 image is expected, got %s' % img_hr_u8.dtype)
    if not img_hr_u8.is_cuda:
        raise RuntimeError('evaluate_image: this path runs only on an MI355X device tensor (got one on %s); there is no CPU '
                           'fallback' % img_hr_u8.device)
    img = img_hr_u8.contiguous()
    H, W, Cimg = (int(v) for v in img.shape)
    s = up.scale
    lr_size = (H // s, W // s) if image_size_lr is None else (int(image_size_lr[0]), int(image_size_lr[1]))
    if (lr_size[0] * s, lr_size[1] * s) != (H, W):
        raise ValueError('evaluate_image: the x%d generator maps a %d x %d LR image to %d x %d, the HR image is %d x %d'
                         % (s, lr_size[0], lr_size[1], lr_size[0] * s, lr_size[1] * s, H, W))
    whole = torch.zeros((1, 4), dtype=torch.int32, device=img.device)            # one window: the image itself
    hr = torch.empty((1, Cimg, H, W), dtype=torch.float32, device=img.device)
    L.check(L.lib().sisr_patch_gather(img.data_ptr(), 1, H, W, Cimg, whole.data_ptr(), 1, H, W, up.mean, up.std, hr.data_ptr(), 0,
                                      _stream()), 'sisr_patch_gather')
    sr = up(lr_from_hr(hr, lr_size)[0])
    p, q = psnr_ssim(sr[None], hr, crop_border=s)
    if niqe_model is None:
        return dict(psnr=p, ssim=q)
    return dict(psnr=p, ssim=q, niqe=niqe(sr[None], niqe_model, crop_border=s))
