"""Differentiable JPEG round trip on the device (csrc/jpeg.hip; the definition is pinned in sisr_hip.h).

Most real low-resolution inputs have been through a JPEG encoder; a generator that never saw 8 x 8 block edges and chroma bleeding
amplifies them.  ``jpeg_roundtrip`` is the encoder + decoder as one operator -- colour transform, 4:2:0 chroma mean, 8 x 8 DCT,
quantisation with libjpeg's tables, and back -- in one launch, differentiable in the image through a surrogate derivative of the
rounding.

>>> y = jpeg_roundtrip(x, 75)                                    # x [N, C, H, W] fp32 in [-1, 1] on the device, C in {1, 3}
>>> y = jpeg_roundtrip(x, q, subsampling='444', grad='cubic')    # q: [N] ints, or explicit tables [N, 2, 8, 8]
>>> d = degrade.Degrader(jpeg=(30, 95))                          # a random quality per sample and per call, drawn on the device

``quant_tables`` / ``expected_quality`` restate the tables and a step's quality draw on the host (no GPU).
"""
import numpy as np
import torch

from . import _lib as L
from .draws import TAG_QUALITY, check_seed_rank, draw_words, uniform24          # TAG_QUALITY: also this module's name for it
from .engine import _stream, require_gpu_tensor

SUBSAMPLING = {'444': L.JPEG_444, '420': L.JPEG_420}
GRAD = {'ste': L.JPEG_GRAD_STE, 'cubic': L.JPEG_GRAD_CUBIC}

# ISO/IEC 10918-1 Annex K, tables K.1 (luminance) and K.2 (chrominance), row-major
BASE_TABLES = np.array([
    [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99],
    [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32],
    dtype=np.int64).reshape(2, 8, 8)


def _check_quality(q, who):
    q = int(q)
    if not 1 <= q <= 100:
        raise ValueError('%s: a quality in [1, 100] is expected, got %d' % (who, q))
    return q


def quant_tables(q):
    """Host: libjpeg's tables at quality ``q`` in [1, 100], in integer arithmetic -> (luma, chroma), two 8 x 8 int64 arrays:
    s = 5000 // q below 50, 200 - 2 q from 50 on; T = clip((base s + 50) // 100, 1, 255)."""
    q = _check_quality(q, 'quant_tables')
    s = 5000 // q if q < 50 else 200 - 2 * q
    t = np.clip((BASE_TABLES * s + 50) // 100, 1, 255)
    return t[0], t[1]


def expected_quality(seed, t, B, qlo, qhi, rank=0):
    """Host restatement of the quality draw of step ``t`` (sisr_jpeg_tables): the first word of the counter tagged
    TAG_QUALITY | rank (draws.py), u0 its 24-bit uniform and the product in fp32 -> int32 numpy array [B]."""
    B, t, (qlo, qhi) = int(B), int(t), check_quality_range((qlo, qhi), 'expected_quality')
    seed, rank = check_seed_rank(seed, rank, 'expected_quality')
    if B < 1 or t < 0:
        raise ValueError('expected_quality: B >= 1 and t >= 0 are expected, got %d, %d' % (B, t))
    u0 = uniform24(draw_words(seed, t, np.arange(B), TAG_QUALITY | rank)[:, 0])
    return np.minimum(qlo + (np.float32(qhi - qlo + 1) * u0).astype(np.int32), qhi).astype(np.int32)


def check_quality_range(jpeg, who):
    qlo, qhi = int(jpeg[0]), int(jpeg[1])
    if not 1 <= qlo <= qhi <= 100:
        raise ValueError('%s: jpeg = (qlo, qhi) needs 1 <= qlo <= qhi <= 100, got (%d, %d)' % (who, qlo, qhi))
    return qlo, qhi


def draw_tables(drawn_step, seed, rank, n, qlo, qhi):
    """One launch (sisr_jpeg_tables): the qualities and quantisation tables of a batch of ``n`` on the step held by ``drawn_step``
    (a 0-dim int64 device tensor, read and NOT advanced) -> (quality [n] int32, tables [n, 2, 8, 8] fp32) on the device"""
    q = torch.empty(n, dtype=torch.int32, device=drawn_step.device)
    tables = torch.empty((n, 2, 8, 8), dtype=torch.float32, device=drawn_step.device)
    L.check(L.lib().sisr_jpeg_tables(drawn_step.data_ptr(), seed, rank, n, qlo, qhi, q.data_ptr(), tables.data_ptr(), _stream()),
            'sisr_jpeg_tables')
    return q, tables


class _JpegRoundTrip(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, tables, sub, grad, clamp):
        n, c, h, w = x.shape
        y = torch.empty_like(x)
        L.check(L.lib().sisr_jpeg_fwd(x.data_ptr(), tables.data_ptr(), y.data_ptr(), n, c, h, w, sub, int(clamp), _stream()),
                'sisr_jpeg_fwd')
        ctx.args = (n, c, h, w, sub, grad, clamp)
        cubic = grad == L.JPEG_GRAD_CUBIC
        ctx.save_for_backward(*((y,) if clamp else ()), *((x, tables) if cubic else ()))
        return y

    @staticmethod
    def backward(ctx, dy):
        n, c, h, w, sub, grad, clamp = ctx.args
        saved = list(ctx.saved_tensors)
        yc = saved.pop(0) if clamp else None
        x, tables = saved if saved else (None, None)
        dy = dy.contiguous()
        dx = torch.empty_like(dy)
        ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
        L.check(L.lib().sisr_jpeg_bwd(dy.data_ptr(), ptr(yc), ptr(x), ptr(tables), dx.data_ptr(), n, c, h, w, sub, grad, _stream()),
                'sisr_jpeg_bwd')
        return dx, None, None, None, None


def _tables_of(quality, n, device):
    """an int, [N] ints or explicit tables [N, 2, 8, 8] -> fp32 [N, 2, 8, 8] on the device.  Qualities are turned into tables on the
    HOST (a device tensor of qualities is read back); explicit tables on the device are used where they lie -- the capturable form."""
    if isinstance(quality, torch.Tensor) and quality.dim() == 4:
        if tuple(quality.shape) != (n, 2, 8, 8):
            raise ValueError('jpeg_roundtrip: tables must be [N = %d, 2, 8, 8], got %s' % (n, tuple(quality.shape)))
        return quality.to(device=device, dtype=torch.float32).contiguous()
    q = np.atleast_1d(np.asarray(quality.cpu() if isinstance(quality, torch.Tensor) else quality))
    if q.ndim != 1 or q.shape[0] not in (1, n) or not np.issubdtype(q.dtype, np.integer):
        raise ValueError('jpeg_roundtrip: quality must be an int, [N = %d] ints or tables [N, 2, 8, 8]' % n)
    t = np.stack([np.stack(quant_tables(v)) for v in q]).astype(np.float32)
    return torch.from_numpy(np.broadcast_to(t, (n, 2, 8, 8)).copy()).to(device)


def jpeg_roundtrip(x, quality, subsampling='420', grad='ste', clamp=True):
    """JPEG-compress and decode ``x`` [N, C, H, W] fp32 in [-1, 1] on the device, C in {1, 3}, any H, W -> the same shape.

    ``quality``      an int in [1, 100], an [N] int tensor, or explicit quantisation tables [N, 2, 8, 8] (luma, chroma; >= 1).
    ``subsampling``  '420' (chroma at half resolution, 16 x 16 MCUs; C = 1 has no chroma and is '444') or '444'.
    ``grad``         the surrogate derivative of the rounding in the backward pass: 'ste' 1, 'cubic' 3 (u - round u)^2.  The forward
                     pass is the hard rounding in both.
    ``clamp``        clamp the decoded image to [-1, 1] (the gradient passes strictly inside).
    Differentiable in ``x`` alone; deterministic (gather form, no atomics).  Not a decoder's bits: libjpeg's integer transforms and
    its smoothing chroma upsampler are left out."""
    require_gpu_tensor(x, 'jpeg_roundtrip input')
    if x.dim() != 4 or x.shape[1] not in (1, 3) or x.dtype != torch.float32:
        raise ValueError('jpeg_roundtrip: an fp32 [N, C, H, W] batch with 1 or 3 channels is expected, got %s %s' % (x.dtype, tuple(x.shape)))
    if subsampling not in SUBSAMPLING or grad not in GRAD:
        raise ValueError("jpeg_roundtrip: subsampling is '444' or '420' and grad 'ste' or 'cubic', got %r, %r" % (subsampling, grad))
    x = x.contiguous()
    return _JpegRoundTrip.apply(x, _tables_of(quality, x.shape[0], x.device), SUBSAMPLING[subsampling], GRAD[grad], bool(clamp))
