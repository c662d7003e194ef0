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

A dataset of MIXED image sizes is packed into one buffer behind a table (``PackedImages``) and sampled by ``RaggedPatchSource``,
every crop inside its own image; ``order='permuted'`` visits every image once per epoch in a new random order each epoch.

>>> packed = PackedImages.from_images(list_of_uint8_HWC_tensors, 'cuda')
>>> src = RaggedPatchSource(packed, 16, (48, 48), crop=(96, 96), hflip=True, order='permuted')
"""
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from .draws import TAG_PERM_BIT, TAG_PERM_KEY, check_seed, draw_words, philox4x32_10  # noqa: F401  (philox4x32_10: its old home)
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
ORDERS = {'random': 0, 'sequential': 1, 'permuted': 2}
OP_HFLIP, OP_VFLIP, OP_TRANSPOSE = 1, 2, 4
PERM_ROUNDS = 24
IMAGE_REC = np.dtype([('offset', '<i8'), ('H', '<i4'), ('W', '<i4')])          # SisrImageRec (sisr_hip.h), 16 bytes


def _mulhi(a, n):
    return (a * np.uint64(n)) >> np.uint64(32)


def permuted_index(seed, epoch, position, M):
    """Pure numpy: sigma_e(p), the swap-or-not shuffle of [0, M) (Hoang, Morris, Rogaway, CRYPTO 2012; sisr_hip.h spells out the
    rounds) keyed by ``seed`` and the epoch alone.  ``epoch`` and ``position`` are integer arrays that broadcast against each
    other -> int64 array of images.  The host restatement of patch_permute in csrc/patchsrc.hip."""
    seed, M = check_seed(seed, 'permuted_index'), int(M)
    e, x = np.broadcast_arrays(np.asarray(epoch, dtype=np.uint64), np.asarray(position, dtype=np.uint64))
    if M < 1 or (x >= np.uint64(M)).any():
        raise ValueError('permuted_index: positions must lie in [0, M = %d)' % M)
    ks = _mulhi(draw_words(seed, e[..., None], np.arange(PERM_ROUNDS), TAG_PERM_KEY)[..., 0].astype(np.uint64), M)      # [..., rounds]
    for r in range(PERM_ROUNDS):
        xp = (ks[..., r] + np.uint64(M) - x) % np.uint64(M)
        bit = draw_words(seed, e, np.maximum(x, xp), TAG_PERM_BIT - r)[..., 0] & 1
        x = np.where(bit == 1, xp, x)
    return x.astype(np.int64)


def _sizes_array(sizes, who):
    a = np.asarray(sizes)
    if a.ndim != 2 or a.shape[1] != 2 or a.shape[0] < 1 or a.dtype.kind not in 'iu':
        raise ValueError('%s: sizes must be an integer [M, 2] array of (H, W), got %s %s' % (who, a.dtype, a.shape))
    return a.astype(np.int64)


def _check_draw_args(B, M, H0, W0, h, w, ops_mask, order, rank, world, who, sizes=None):
    """``sizes``: [M, 2] int64 (H, W) of a ragged dataset, which replace H0 and W0"""
    if min(B, M, h, w) < 1 or (sizes is None and min(H0, W0) < 1):
        raise ValueError('%s: sizes must be >= 1, got B %d, M %d, image %d x %d, window %d x %d' % (who, B, M, H0, W0, h, w))
    if sizes is None:
        if h > H0 or w > W0:
            raise ValueError('%s: the %d x %d window is larger than the %d x %d image' % (who, h, w, H0, W0))
    else:
        if sizes.shape[0] != M:
            raise ValueError('%s: %d sizes for %d images' % (who, sizes.shape[0], M))
        small = np.nonzero((sizes[:, 0] < h) | (sizes[:, 1] < w))[0]
        if small.size:
            i = int(small[0])
            raise ValueError('%s: the %d x %d window is larger than image %d (%d x %d)' % (who, h, w, i, sizes[i, 0], sizes[i, 1]))
    if order not in ORDERS:
        raise ValueError("%s: order must be 'random', 'sequential' or 'permuted', got %r" % (who, order))
    if world < 1 or not 0 <= rank < world:
        raise ValueError('%s: rank %d is not in [0, world = %d)' % (who, rank, world))
    if not 0 <= ops_mask <= 7:
        raise ValueError('%s: ops_mask must be in [0, 7], got %d' % (who, ops_mask))
    if ops_mask & OP_TRANSPOSE and h != w:
        raise ValueError('%s: transposition needs a square window, got %d x %d' % (who, h, w))
    if order != 'random' and M < B * world:
        raise ValueError('%s: %s order over %d images has no full batch of %d x %d ranks' % (who, order, M, B, world))


def expected_draws(seed, t, B, M, H0, W0, h, w, ops_mask, order='random', rank=0, world=1, sizes=None):
    """Pure numpy: the [B, 4] int32 draw table (index, y0, x0, ops) of step ``t`` -- what sisr_patch_draw / sisr_patch_draw_table
    write and sisr_patch_draws_host / sisr_patch_draws_table_host compute.  ``sizes``: [M, 2] (H, W) of a ragged dataset (H0 and
    W0 are then not read).  For audits and tests."""
    t = int(t)
    B, M, H0, W0, h, w, ops_mask, rank, world = (int(v) for v in (B, M, H0, W0, h, w, ops_mask, rank, world))
    if sizes is not None:
        sizes = _sizes_array(sizes, 'expected_draws')
    _check_draw_args(B, M, H0, W0, h, w, ops_mask, order, rank, world, 'expected_draws', sizes)
    seed = check_seed(seed, 'expected_draws')
    if t < 0:
        raise ValueError('expected_draws: t must be >= 0, got %d' % t)
    b = np.arange(B, dtype=np.uint64)
    r = draw_words(seed, t, b, rank).astype(np.uint64)
    if order == 'random':
        index = _mulhi(r[:, 0], M)
    else:
        nb = M // (B * world)
        index = ((t % nb) * world + rank) * B + b
        if order == 'permuted':
            index = permuted_index(seed, t // nb, index, M).astype(np.uint64)
    if sizes is None:
        ry, rx = np.uint64(H0 - h + 1), np.uint64(W0 - w + 1)
    else:
        ry, rx = ((sizes[index.astype(np.int64), k] - n + 1).astype(np.uint64) for k, n in ((0, h), (1, w)))
    out = np.stack([index, (r[:, 1] * ry) >> np.uint64(32), (r[:, 2] * rx) >> np.uint64(32), r[:, 3] & np.uint64(ops_mask)], axis=-1)
    return out.astype(np.int32)


def image_table(sizes, C, align=16):
    """Pure host: the table of a packed store that holds images of ``sizes`` ([M, 2] of (H, W)) with ``C`` channels one after the
    other, each offset aligned up to ``align`` bytes -> (table: [M] numpy records of IMAGE_REC, bytes the buffer needs)"""
    sizes, C, align = _sizes_array(sizes, 'image_table'), int(C), int(align)
    if not 1 <= C <= 4:
        raise ValueError('image_table: 1 to 4 channels are supported, got %d' % C)
    if align < 1:
        raise ValueError('image_table: align must be >= 1, got %d' % align)
    table = np.zeros(sizes.shape[0], dtype=IMAGE_REC)
    end = 0
    for i, (H, W) in enumerate(sizes.tolist()):
        if H < 1 or W < 1:
            raise ValueError('image_table: image %d is %d x %d; sizes must be >= 1' % (i, H, W))
        at = -(-end // align) * align
        table[i] = (at, H, W)
        end = at + H * W * C
    return table, end


def _check_image_table(table, C, data_bytes, who):
    """-> [M] IMAGE_REC records; ValueError naming the first image that breaks the rules of a packed store"""
    t = np.asarray(table)
    if t.dtype != IMAGE_REC:
        if t.ndim != 2 or t.shape[1] != 3 or t.dtype.kind not in 'iu':
            raise ValueError('%s: the table must be [M] records of IMAGE_REC or an integer [M, 3] array of (offset, H, W), got %s %s'
                             % (who, t.dtype, t.shape))
        rec = np.zeros(t.shape[0], dtype=IMAGE_REC)
        if t.size and (np.abs(t[:, 1:].astype(np.int64)) >= 1 << 31).any():
            raise ValueError('%s: an image size does not fit 32 bits' % who)
        rec['offset'], rec['H'], rec['W'] = t[:, 0], t[:, 1], t[:, 2]
        t = rec
    if t.ndim != 1 or t.shape[0] < 1 or t.shape[0] >= 1 << 31:
        raise ValueError('%s: a table of 1 to 2^31 - 1 images is expected, got shape %s' % (who, t.shape))
    if not 1 <= C <= 4:
        raise ValueError('%s: 1 to 4 channels are supported, got %d' % (who, C))
    off, H, W = t['offset'].astype(np.int64), t['H'].astype(np.int64), t['W'].astype(np.int64)
    end = off + H * W * C
    for i in np.nonzero((H < 1) | (W < 1) | (off < 0) | (end > data_bytes))[0][:1].tolist():
        raise ValueError('%s: image %d (offset %d, %d x %d x %d) has a size < 1, a negative offset or ends past the %d bytes of data'
                         % (who, i, off[i], H[i], W[i], C, data_bytes))
    by_offset = np.argsort(off, kind='stable')
    for k in np.nonzero(end[by_offset][:-1] > off[by_offset][1:])[0][:1].tolist():
        i, j = sorted((int(by_offset[k]), int(by_offset[k + 1])))
        raise ValueError('%s: image %d (offset %d, %d x %d x %d) overlaps image %d' % (who, j, off[j], H[j], W[j], C, i))
    return np.ascontiguousarray(t)


class PackedImages:
    """M decoded images of their own sizes in ONE contiguous uint8 device buffer, image i as [H_i, W_i, C] row-interleaved bytes at
    ``table[i].offset``, and the table of SisrImageRec { int64 offset; int32 H; int32 W } on the device beside it (DESIGN.md
    section 12).  The table is validated on the host, once, here: sizes >= 1, offsets >= 0, every image inside the buffer, no two
    images overlapping (gaps are fine), 1 <= C <= 4 -- ValueError names the first offender.

    ``data`` uint8 [bytes] and ``table`` on the device, ``table_host`` the numpy records, ``sizes`` [M, 2] int64 (H, W), ``C``."""

    def __init__(self, data_u8, table_host, C):
        """use from_images / from_packed"""
        self.data, self.table_host, self.C = data_u8, table_host, C
        self.sizes = np.stack([table_host['H'], table_host['W']], axis=-1).astype(np.int64)
        self.table = torch.from_numpy(table_host.view(np.uint8).copy()).to(data_u8.device)

    def __len__(self):
        return self.table_host.shape[0]

    @classmethod
    def from_packed(cls, data_u8, table_host, C=3):
        """``data_u8``: flat uint8 device tensor, held by reference; ``table_host``: [M] records of IMAGE_REC (or an integer
        [M, 3] array of offset, H, W) built by the caller -- image_table() builds the gapless one"""
        refuse = lambda: RuntimeError('PackedImages: a contiguous 1-D uint8 buffer on the MI355X is expected (got %s %s on %s); there '
                                      'is no CPU fallback' % (getattr(data_u8, 'dtype', type(data_u8)),
                                                              tuple(getattr(data_u8, 'shape', ())), getattr(data_u8, 'device', '?')))
        if not (isinstance(data_u8, torch.Tensor) and data_u8.dtype == torch.uint8 and data_u8.dim() == 1):
            raise refuse()
        table = _check_image_table(table_host, int(C), data_u8.numel(), 'PackedImages.from_packed')
        if not (data_u8.is_cuda and data_u8.is_contiguous()):              # after the checks that need the shapes alone
            raise refuse()
        return cls(data_u8, table, int(C))

    @classmethod
    def from_images(cls, images, device):
        """``images``: a list of uint8 [H, W, C] tensors (host or device) of one C; copied one after the other, every offset
        aligned up to 16 bytes, into a new buffer on ``device``"""
        images = list(images)
        for i, im in enumerate(images):
            if not (isinstance(im, torch.Tensor) and im.dtype == torch.uint8 and im.dim() == 3):
                raise RuntimeError('PackedImages.from_images: image %d is not a uint8 [H, W, C] tensor (got %s %s)'
                                   % (i, getattr(im, 'dtype', type(im)), tuple(getattr(im, 'shape', ()))))
        if not images:
            raise ValueError('PackedImages.from_images: no images')
        C = int(images[0].shape[2])
        for i, im in enumerate(images):
            if im.shape[2] != C:
                raise ValueError('PackedImages.from_images: image %d has %d channels, image 0 has %d' % (i, im.shape[2], C))
        table, total = image_table([tuple(im.shape[:2]) for im in images], C)
        device = torch.device(device)
        if device.type != 'cuda':
            raise RuntimeError('PackedImages.from_images: the store lives on the MI355X (got device %s); there is no CPU fallback' % device)
        data = torch.zeros(total, dtype=torch.uint8, device=device)
        for rec, im in zip(table.tolist(), images):
            data[rec[0]:rec[0] + im.numel()].copy_(im.reshape(-1))
        return cls(data, table, C)


class _PatchSource:
    """what DevicePatchSource and RaggedPatchSource share: the call contract around their two pairs of entry points.  A subclass
    sets images-independent state through _setup() and supplies _M(), _sizes() (None: uniform H0 x W0), _draw() and _launch_gather()."""

    def _setup(self, dev, C, batch_size, window, image_size_lr, resize, hflip, vflip, transpose, order, seed, rank, world, mean, std,
               check_device):
        who = type(self).__name__
        self.C, self.B, self.window = C, int(batch_size), window
        self.ops_mask = (OP_HFLIP if hflip else 0) | (OP_VFLIP if vflip else 0) | (OP_TRANSPOSE if transpose else 0)
        self.order, self.rank, self.world = order, int(rank), int(world)
        self._check(order, self.rank, self.world, who)
        self.seed = check_seed(seed, who)
        if float(std) == 0.0:
            raise ValueError('%s: std must not be 0' % who)
        check_device()                                                     # after the checks that need the shape alone
        self.lr = (int(image_size_lr[0]), int(image_size_lr[1]))
        self.mean, self.std = float(mean), float(std)
        self.resize = None if resize is None else (int(resize[0]), int(resize[1]))
        self._dev = dev
        self._step = torch.zeros((), dtype=torch.int64, device=dev)
        self._draws = torch.zeros((self.B, 4), dtype=torch.int32, device=dev)
        self._pipe, self._u8 = None, None
        if self.resize is not None:
            self._pipe = PatchPipeline(self.resize, self.lr, self.mean, self.std)
            self._u8 = torch.empty((self.B,) + self.window + (C,), dtype=torch.uint8, device=dev)
            for n_in, n_out in zip(self.window, self.resize):          # coefficient tables: host work and a copy, done now
                if n_in != n_out:
                    self._pipe._axis(n_in, n_out, dev)

    def _check(self, order, rank, world, who):
        H0, W0 = self._uniform_size()
        _check_draw_args(self.B, self._M(), H0, W0, self.window[0], self.window[1], self.ops_mask, order, rank, world, who, self._sizes())

    @property
    def step_count(self):
        """0-dim int64 device tensor: batches drawn so far (reading it is the caller's synchronisation)"""
        return self._step

    @property
    def last_draws(self):
        """[B, 4] int32 device tensor (index, y0, x0, ops) of the latest call"""
        return self._draws

    @property
    def epoch_length(self):
        """host int nb = M // (B * world): batches per epoch of the sequential and permuted orders"""
        return self._M() // (self.B * self.world)

    def _gather(self, draws, n, u8_out):
        h, w = self.window
        if self.resize is None:
            out, kind = torch.empty((n, self.C, h, w), dtype=torch.float32, device=self._dev), 0
        else:
            out, kind = u8_out, 1
        self._launch_gather(draws, n, out, kind)
        return out if self.resize is None else self._pipe.resize_normalize(out)

    def __call__(self):
        self._draw()
        img_hr = self._gather(self._draws, self.B, self._u8)
        return img_hr, lr_from_hr(img_hr, self.lr)

    def gather(self, draws):
        """The gather (and resize) of ``src()`` for a table written by hand: ``draws`` is a host int array or tensor [n, 4] of
        (index, y0, x0, ops) rows, validated on the host (every row against its own image's size) -> img_hr [n, C, H, W]"""
        who = type(self).__name__
        rows = np.asarray(draws.cpu() if isinstance(draws, torch.Tensor) else draws)
        if rows.ndim != 2 or rows.shape[1] != 4 or rows.shape[0] < 1 or rows.dtype.kind not in 'iu':
            raise ValueError('%s.gather: an integer [n, 4] table is expected, got %s %s' % (who, rows.dtype, rows.shape))
        rows = rows.astype(np.int64)
        M, sizes, (h, w) = self._M(), self._sizes(), self.window
        for k, (i, y0, x0, ops) in enumerate(rows.tolist()):
            H0, W0 = self._uniform_size() if sizes is None or not 0 <= i < M else sizes[i].tolist()
            if not (0 <= i < M and 0 <= y0 <= H0 - h and 0 <= x0 <= W0 - w and 0 <= ops <= 7) or (ops & OP_TRANSPOSE and h != w):
                raise ValueError('%s.gather: row %d (index %d, y0 %d, x0 %d, ops %d) is out of range for %d images '
                                 'of %d x %d and a %d x %d window' % (who, k, i, y0, x0, ops, M, H0, W0, h, w))
        table = torch.from_numpy(rows.astype(np.int32)).to(self._dev)
        n = table.shape[0]
        u8 = None if self.resize is None else torch.empty((n, h, w, self.C), dtype=torch.uint8, device=self._dev)
        return self._gather(table, n, u8)

    def state_dict(self):
        return dict(seed=self.seed, step_count=self._step.clone(), order=self.order, rank=self.rank, world=self.world)

    def load_state_dict(self, state):
        """copies the count INTO the existing tensor (a captured draw points at it)"""
        who = type(self).__name__ + '.load_state_dict'
        order, rank, world = state['order'], int(state['rank']), int(state['world'])
        self._check(order, rank, world, who)
        seed = check_seed(state['seed'], who)
        self._step.copy_(torch.as_tensor(state['step_count'], dtype=torch.int64).reshape(()))
        self.order, self.rank, self.world, self.seed = order, rank, world, seed


class DevicePatchSource(_PatchSource):
    """Batches sampled on the device from a device-resident decoded dataset (module docstring).

    ``images_u8``  [M, H0, W0, C] uint8, contiguous, on the device; held by reference, never copied.
    ``crop``       (h, w) window drawn uniformly inside each image; None: the whole image (offsets always 0).
    ``resize``     (H, W): the windows go through the reference's Resize + ToTensor + Normalize (PatchPipeline's kernel,
                   bit-exact with Pillow); None: ToTensor + Normalize alone.
    ``hflip`` / ``vflip`` / ``transpose``  each switched-on operation is applied to a sample with probability 1/2, in this order.
    ``order``      'random': images i.i.d. with replacement; 'sequential': the reference's sampler (images in order, the last
                   partial batch dropped, rank r of ``world`` takes every world-th batch); 'permuted': the sequential positions
                   read through a permutation of the images that is new every epoch and the same on every rank (each image at
                   most once per epoch; the M mod (B * world) left-over images change from epoch to epoch).  Windows and
                   operations are random in every order.  ``epoch_length`` is the number of batches per epoch.
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

        def check_device():
            if not (images_u8.is_cuda and images_u8.is_contiguous()):
                raise refuse()
        self._setup(images_u8.device, C, batch_size, (H0, W0) if crop is None else (int(crop[0]), int(crop[1])), image_size_lr,
                    resize, hflip, vflip, transpose, order, seed, rank, world, mean, std, check_device)

    def _M(self):
        return int(self.images.shape[0])

    def _sizes(self):
        return None

    def _uniform_size(self):
        return int(self.images.shape[1]), int(self.images.shape[2])

    def _draw(self):
        M, H0, W0, _ = self.images.shape
        lib, head = L.lib(), (self._step.data_ptr(), self.seed, self.rank, self.world, ORDERS[self.order], self.B, M, H0, W0)
        tail = (self.window[0], self.window[1], self.ops_mask, self._draws.data_ptr(), _stream())
        if self.order == 'permuted':              # the one order the first entry point does not know
            L.check(lib.sisr_patch_draw_table(*head, None, *tail), 'sisr_patch_draw_table')
        else:
            L.check(lib.sisr_patch_draw(*head, *tail), 'sisr_patch_draw')

    def _launch_gather(self, draws, n, out, kind):
        M, H0, W0, C = self.images.shape
        L.check(L.lib().sisr_patch_gather(self.images.data_ptr(), M, H0, W0, C, draws.data_ptr(), n, self.window[0], self.window[1],
                                          self.mean, self.std, out.data_ptr(), kind, _stream()), 'sisr_patch_gather')


class RaggedPatchSource(_PatchSource):
    """DevicePatchSource over a PackedImages store: images of mixed sizes, every window drawn uniformly inside ITS image (the
    standard random-crop recipe of super-resolution training sets).  Same arguments, same call contract -- ``src()``,
    ``last_draws``, ``step_count``, ``epoch_length``, ``gather(draws)``, ``state_dict`` / ``load_state_dict``, usable inside
    graph.GraphedStep with no warm-up of its own -- except that ``crop`` is required: the window is one size for the whole batch
    (and the resize tables depend on it), and an image smaller than it is refused here, by name.  Images are drawn uniformly
    whatever their area."""

    def __init__(self, packed, batch_size, image_size_lr, *, crop, resize=None, hflip=False, vflip=False, transpose=False,
                 order='random', seed=0, rank=0, world=1, mean=0.5, std=0.5):
        if not isinstance(packed, PackedImages):
            raise RuntimeError('RaggedPatchSource: a PackedImages store is expected, got %s' % type(packed))
        if crop is None:
            raise ValueError('RaggedPatchSource: crop=(h, w) is required: images of mixed sizes have no common whole-image window')
        self.packed = packed

        def check_device():
            if not packed.data.is_cuda:
                raise RuntimeError('RaggedPatchSource: a store on the MI355X is expected (got one on %s); there is no CPU fallback'
                                   % packed.data.device)
        self._setup(packed.data.device, packed.C, batch_size, (int(crop[0]), int(crop[1])), image_size_lr, resize, hflip, vflip,
                    transpose, order, seed, rank, world, mean, std, check_device)

    def _M(self):
        return len(self.packed)

    def _sizes(self):
        return self.packed.sizes

    def _uniform_size(self):
        return 0, 0

    def _draw(self):
        L.check(L.lib().sisr_patch_draw_table(self._step.data_ptr(), self.seed, self.rank, self.world, ORDERS[self.order], self.B,
                                              self._M(), 0, 0, self.packed.table.data_ptr(), self.window[0], self.window[1],
                                              self.ops_mask, self._draws.data_ptr(), _stream()), 'sisr_patch_draw_table')

    def _launch_gather(self, draws, n, out, kind):
        p = self.packed
        L.check(L.lib().sisr_patch_gather_table(p.data.data_ptr(), p.data.numel(), p.table.data_ptr(), self._M(), p.C, draws.data_ptr(),
                                                n, self.window[0], self.window[1], self.mean, self.std, out.data_ptr(), kind,
                                                _stream()), 'sisr_patch_gather_table')
