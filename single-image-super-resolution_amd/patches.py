"""On-device patch pipeline: what happens to every image between the decoder and the generator.

The reference transforms each decoded image on the host, one at a time, inside its DataLoader workers
(config.py:225-231: ``transforms.Resize(image_size_hr[1:])`` -- Pillow's anti-aliased BILINEAR resize of the 8-bit
image --, ``ToTensor()``, ``Normalize((.5, .5, .5), (.5, .5, .5))``), moves the float batch to the device
(train.py:45) and degrades it there (train.py:46 ``utils.lr_from_hr``).  ``PatchPipeline`` takes the batch of DECODED
images as uint8 on the device (a quarter of the float bytes over PCIe) and produces both ``img_hr`` and ``img_lr``
there: one launch for Resize + ToTensor + Normalize (csrc/resample.hip, integer arithmetic bit-exact with Pillow),
one for the bicubic degradation + clamp (the kernel behind ``utils.lr_from_hr``), which reads ``img_hr`` back out of
L2.  ``img_hr`` has to be materialised anyway: it is the discriminator's real batch and the content-loss target.

>>> pipe = PatchPipeline(image_size_hr[1:], image_size_lr[1:])
>>> img_hr, img_lr = pipe(batch_u8.to(device))          # batch_u8: [B, H0, W0, C] uint8, e.g. CelebA 218 x 178 x 3

``DevicePatchSource`` removes the remaining host work of an iteration: the whole DECODED dataset lives on the
device ([M, H0, W0, C] uint8: CelebA is 23.6 GB of the card's 288 GB) and every batch is sampled from it there -- which image,
which crop window, which flip / transposition -- by two launches whose step count is device memory, so the input side of an
iteration can be captured into the same HIP graph as the rest and still produce a new batch on every replay.

>>> src = DevicePatchSource(dataset_u8, 16, (48, 48), crop=(96, 96), hflip=True)          # dataset_u8 on the device
>>> img_hr, img_lr = src()
"""
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from .engine import _stream
from .utils import lr_from_hr


class PatchPipeline:
    def __init__(self, image_size_hr, image_size_lr, mean=0.5, std=0.5):
        self.hr, self.lr = (int(image_size_hr[0]), int(image_size_hr[1])), (int(image_size_lr[0]), int(image_size_lr[1]))
        self.mean, self.std = float(mean), float(std)
        self._tables = {}                  # (axis input size, output size, device) -> (bounds, kk, ksize) on the device

    def _axis(self, n_in, n_out, dev):
        key = (n_in, n_out, str(dev))
        if key not in self._tables:
            lib = L.lib()
            ks = L.check_count(lib.sisr_resize_coeffs(n_in, n_out, None, None), 'sisr_resize_coeffs')
            bounds = np.zeros((n_out, 2), dtype=np.int32)
            kk = np.zeros((n_out, ks), dtype=np.int32)
            L.check_count(lib.sisr_resize_coeffs(n_in, n_out, bounds.ctypes.data_as(C.c_void_p), kk.ctypes.data_as(C.c_void_p)),
                          'sisr_resize_coeffs')
            self._tables[key] = (torch.from_numpy(bounds).to(dev), torch.from_numpy(kk).to(dev), ks)
        return self._tables[key]

    def resize_normalize(self, imgs_u8):
        """transforms.Resize + ToTensor + Normalize of config.py:225-231 on a batch: [N, H0, W0, C] uint8 -> [N, C, H, W] float32"""
        if not (isinstance(imgs_u8, torch.Tensor) and imgs_u8.is_cuda and imgs_u8.dtype == torch.uint8 and imgs_u8.dim() == 4):
            raise RuntimeError('PatchPipeline: a [N, H0, W0, C] uint8 batch on the MI355X is expected (got %s %s on %s); there is no '
                               'CPU fallback' % (getattr(imgs_u8, 'dtype', type(imgs_u8)), tuple(getattr(imgs_u8, 'shape', ())),
                                                 getattr(imgs_u8, 'device', '?')))
        x = imgs_u8.contiguous()
        n, h0, w0, c = x.shape
        h, w = self.hr
        out = torch.empty((n, c, h, w), dtype=torch.float32, device=x.device)
        bx, kx, ksx = self._axis(w0, w, x.device) if w0 != w else (None, None, 0)
        by, ky, ksy = self._axis(h0, h, x.device) if h0 != h else (None, None, 0)
        ptr = lambda t: None if t is None else t.data_ptr()
        L.check(L.lib().sisr_resize_u8_normalize(x.data_ptr(), out.data_ptr(), n, h0, w0, c, h, w, ptr(bx), ptr(kx), ksx,
                                                 ptr(by), ptr(ky), ksy, self.mean, self.std, _stream()),
                'sisr_resize_u8_normalize')
        return out

    def __call__(self, imgs_u8):
        img_hr = self.resize_normalize(imgs_u8)
        return img_hr, lr_from_hr(img_hr, self.lr)            # train.py:46


# ---- device-resident patch source ------------------------------------------------------------------------------------------------
ORDERS = {'random': 0, 'sequential': 1}
OP_HFLIP, OP_VFLIP, OP_TRANSPOSE = 1, 2, 4
_M32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., SC'11) in numpy.  counter: [..., 4], key: [..., 2] words (broadcast against each other) ->
    [..., 4] uint32.  The host restatement of the generator in csrc/patchsrc.hip."""
    c = np.asarray(counter, dtype=np.uint64) & _M32
    k = np.asarray(key, dtype=np.uint64) & _M32
    c0, c1, c2, c3 = (c[..., i] for i in range(4))
    k0, k1 = k[..., 0], k[..., 1]
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2           # 32 x 32 -> 64 bits: exact in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M32, (k1 + np.uint64(0xBB67AE85)) & _M32
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1).astype(np.uint32)


def _check_draw_args(B, M, H0, W0, h, w, ops_mask, order, rank, world, who):
    if min(B, M, H0, W0, h, w) < 1:
        raise ValueError('%s: sizes must be >= 1, got B %d, M %d, image %d x %d, window %d x %d' % (who, B, M, H0, W0, h, w))
    if h > H0 or w > W0:
        raise ValueError('%s: the %d x %d window is larger than the %d x %d image' % (who, h, w, H0, W0))
    if order not in ORDERS:
        raise ValueError("%s: order must be 'random' or 'sequential', got %r" % (who, order))
    if world < 1 or not 0 <= rank < world:
        raise ValueError('%s: rank %d is not in [0, world = %d)' % (who, rank, world))
    if not 0 <= ops_mask <= 7:
        raise ValueError('%s: ops_mask must be in [0, 7], got %d' % (who, ops_mask))
    if ops_mask & OP_TRANSPOSE and h != w:
        raise ValueError('%s: transposition needs a square window, got %d x %d' % (who, h, w))
    if order == 'sequential' and M < B * world:
        raise ValueError('%s: sequential order over %d images has no full batch of %d x %d ranks' % (who, M, B, world))


def expected_draws(seed, t, B, M, H0, W0, h, w, ops_mask, order='random', rank=0, world=1):
    """Pure numpy: the [B, 4] int32 draw table (index, y0, x0, ops) of step ``t`` -- what sisr_patch_draw writes and
    sisr_patch_draws_host computes.  For audits and tests."""
    seed, t = int(seed), int(t)
    B, M, H0, W0, h, w, ops_mask, rank, world = (int(v) for v in (B, M, H0, W0, h, w, ops_mask, rank, world))
    _check_draw_args(B, M, H0, W0, h, w, ops_mask, order, rank, world, 'expected_draws')
    if t < 0 or not 0 <= seed < 1 << 64:
        raise ValueError('expected_draws: t must be >= 0 and seed in [0, 2^64), got t %d, seed %d' % (t, seed))
    b = np.arange(B, dtype=np.uint64)
    ctr = np.stack([np.full(B, t & _M32, np.uint64), np.full(B, (t >> 32) & _M32, np.uint64), b, np.full(B, rank, np.uint64)], axis=-1)
    r = philox4x32_10(ctr, np.array([seed & _M32, seed >> 32], dtype=np.uint64)).astype(np.uint64)
    mulhi = lambda a, n: (a * np.uint64(n)) >> np.uint64(32)
    if order == 'sequential':
        nb = M // (B * world)
        index = ((t % nb) * world + rank) * B + b
    else:
        index = mulhi(r[:, 0], M)
    out = np.stack([index, mulhi(r[:, 1], H0 - h + 1), mulhi(r[:, 2], W0 - w + 1), r[:, 3] & np.uint64(ops_mask)], axis=-1)
    return out.astype(np.int32)


class DevicePatchSource:
    """Batches sampled on the device from a device-resident decoded dataset (module docstring).

    ``images_u8``  [M, H0, W0, C] uint8, contiguous, on the device; held by reference, never copied.
    ``crop``       (h, w) window drawn uniformly inside each image; None: the whole image (offsets always 0).
    ``resize``     (H, W): the windows go through the reference's Resize + ToTensor + Normalize (PatchPipeline's kernel,
                   bit-exact with Pillow); None: ToTensor + Normalize alone.
    ``hflip`` / ``vflip`` / ``transpose``  each switched-on operation is applied to a sample with probability 1/2, in this order.
    ``order``      'random': images i.i.d. with replacement; 'sequential': the reference's sampler (images in order, the last
                   partial batch dropped, rank r of ``world`` takes every world-th batch), windows and operations still random.
    ``crop=None, resize=image_size_hr, order='sequential'`` with no operation is the reference's input side (config.py:225-251,
    train.py:45-46).

    ``src()`` -> (img_hr, img_lr): two launches (draw, gather), a third with ``resize``, then utils.lr_from_hr.  Everything but
    the outputs exists from construction on and the step count lives on the device: ``src()`` may be called inside
    graph.GraphedStep with no warm-up of its own, and every replay produces the next batch."""

    def __init__(self, images_u8, batch_size, image_size_lr, *, crop=None, resize=None, hflip=False, vflip=False, transpose=False,
                 order='random', seed=0, rank=0, world=1, mean=0.5, std=0.5):
        refuse = lambda: RuntimeError('DevicePatchSource: a contiguous [M, H0, W0, C] uint8 dataset on the MI355X is expected (got %s %s '
                                      'on %s); there is no CPU fallback' % (getattr(images_u8, 'dtype', type(images_u8)),
                                                                            tuple(getattr(images_u8, 'shape', ())),
                                                                            getattr(images_u8, 'device', '?')))
        if not (isinstance(images_u8, torch.Tensor) and images_u8.dtype == torch.uint8 and images_u8.dim() == 4):
            raise refuse()
        self.images = images_u8
        M, H0, W0, C = (int(v) for v in images_u8.shape)
        if not 1 <= C <= 4:
            raise ValueError('DevicePatchSource: 1 to 4 channels are supported, got %d' % C)
        self.B = int(batch_size)
        self.window = (H0, W0) if crop is None else (int(crop[0]), int(crop[1]))
        self.ops_mask = (OP_HFLIP if hflip else 0) | (OP_VFLIP if vflip else 0) | (OP_TRANSPOSE if transpose else 0)
        self.order, self.seed, self.rank, self.world = order, int(seed), int(rank), int(world)
        _check_draw_args(self.B, M, H0, W0, self.window[0], self.window[1], self.ops_mask, order, self.rank, self.world,
                         'DevicePatchSource')
        if not 0 <= self.seed < 1 << 64:
            raise ValueError('DevicePatchSource: seed must be in [0, 2^64), got %d' % self.seed)
        if float(std) == 0.0:
            raise ValueError('DevicePatchSource: std must not be 0')
        if not (images_u8.is_cuda and images_u8.is_contiguous()):          # after the checks that need the shape alone
            raise refuse()
        self.lr = (int(image_size_lr[0]), int(image_size_lr[1]))
        self.mean, self.std = float(mean), float(std)
        self.resize = None if resize is None else (int(resize[0]), int(resize[1]))
        dev = images_u8.device
        self._step = torch.zeros((), dtype=torch.int64, device=dev)
        self._draws = torch.zeros((self.B, 4), dtype=torch.int32, device=dev)
        self._pipe, self._u8 = None, None
        if self.resize is not None:
            self._pipe = PatchPipeline(self.resize, self.lr, self.mean, self.std)
            self._u8 = torch.empty((self.B,) + self.window + (C,), dtype=torch.uint8, device=dev)
            for n_in, n_out in zip(self.window, self.resize):          # coefficient tables: host work and a copy, done now
                if n_in != n_out:
                    self._pipe._axis(n_in, n_out, dev)

    @property
    def step_count(self):
        """0-dim int64 device tensor: batches drawn so far (reading it is the caller's synchronisation)"""
        return self._step

    @property
    def last_draws(self):
        """[B, 4] int32 device tensor (index, y0, x0, ops) of the latest call"""
        return self._draws

    def _gather(self, draws, n, u8_out):
        M, H0, W0, C = self.images.shape
        h, w = self.window
        if self.resize is None:
            out, kind = torch.empty((n, C, h, w), dtype=torch.float32, device=self.images.device), 0
        else:
            out, kind = u8_out, 1
        L.check(L.lib().sisr_patch_gather(self.images.data_ptr(), M, H0, W0, C, draws.data_ptr(), n, h, w, self.mean, self.std,
                                          out.data_ptr(), kind, _stream()), 'sisr_patch_gather')
        return out if self.resize is None else self._pipe.resize_normalize(out)

    def __call__(self):
        M, H0, W0, _ = self.images.shape
        L.check(L.lib().sisr_patch_draw(self._step.data_ptr(), self.seed, self.rank, self.world, ORDERS[self.order], self.B, M, H0, W0,
                                        self.window[0], self.window[1], self.ops_mask, self._draws.data_ptr(), _stream()),
                'sisr_patch_draw')
        img_hr = self._gather(self._draws, self.B, self._u8)
        return img_hr, lr_from_hr(img_hr, self.lr)

    def gather(self, draws):
        """The gather (and resize) of ``src()`` for a table written by hand: ``draws`` is a host int array or tensor [n, 4] of
        (index, y0, x0, ops) rows, validated on the host -> img_hr [n, C, H, W]"""
        rows = np.asarray(draws.cpu() if isinstance(draws, torch.Tensor) else draws)
        if rows.ndim != 2 or rows.shape[1] != 4 or rows.shape[0] < 1 or rows.dtype.kind not in 'iu':
            raise ValueError('DevicePatchSource.gather: an integer [n, 4] table is expected, got %s %s' % (rows.dtype, rows.shape))
        rows = rows.astype(np.int64)
        M, H0, W0, C = self.images.shape
        h, w = self.window
        for k, (i, y0, x0, ops) in enumerate(rows.tolist()):
            if not (0 <= i < M and 0 <= y0 <= H0 - h and 0 <= x0 <= W0 - w and 0 <= ops <= 7) or (ops & OP_TRANSPOSE and h != w):
                raise ValueError('DevicePatchSource.gather: row %d (index %d, y0 %d, x0 %d, ops %d) is out of range for %d images '
                                 'of %d x %d and a %d x %d window' % (k, i, y0, x0, ops, M, H0, W0, h, w))
        dev = self.images.device
        table = torch.from_numpy(rows.astype(np.int32)).to(dev)
        n = table.shape[0]
        u8 = None if self.resize is None else torch.empty((n, h, w, C), dtype=torch.uint8, device=dev)
        return self._gather(table, n, u8)

    def state_dict(self):
        return dict(seed=self.seed, step_count=self._step.clone(), order=self.order, rank=self.rank, world=self.world)

    def load_state_dict(self, state):
        """copies the count INTO the existing tensor (a captured draw points at it)"""
        order, rank, world, seed = state['order'], int(state['rank']), int(state['world']), int(state['seed'])
        M, H0, W0, _ = self.images.shape
        _check_draw_args(self.B, M, H0, W0, self.window[0], self.window[1], self.ops_mask, order, rank, world,
                         'DevicePatchSource.load_state_dict')
        if not 0 <= seed < 1 << 64:
            raise ValueError('DevicePatchSource.load_state_dict: seed must be in [0, 2^64), got %d' % seed)
        self._step.copy_(torch.as_tensor(state['step_count'], dtype=torch.int64).reshape(()))
        self.order, self.rank, self.world, self.seed = order, rank, world, seed
