"""GPU: the patch source over images of mixed sizes and the permuted order (patches.PackedImages, patches.RaggedPatchSource,
csrc/patchsrc.hip).

The reference is that of test_gpu_patchsrc.py, torch on the CPU, written here over a LIST of images: slice the window out of the
drawn image, flip(1) for bit 0, flip(0) for bit 1, transpose(0, 1) for bit 2, permute to CHW, ``.float() / 255``,
``(t - mean) / std``.  Kernel and reference perform the same two correctly rounded fp32 operations on the same 8-bit value, so
the bound is bit-equality (torch.equal).  With ``resize=`` the uint8 windows cut by hand go through the existing
PatchPipeline.resize_normalize, which test_gpu_patches.py holds to Pillow: bit-equality again.

The gather kernel's tile is 32 x 32 window pixels: the 33 x 33, 67 x 65 and 70 x 70 windows span 2 x 2 and 3 x 3 tiles with ragged
remainders of 1, 3 and 6 pixels."""
import numpy as np
import pytest
import torch

from gpu_helpers import pkg

pytestmark = pytest.mark.gpu

SIZES = ((4, 4), (7, 9), (33, 65), (70, 70), (67, 131))
RESIZE = (6, 5)


def _images(sizes, C, start=0):
    """arange-like: neighbouring bytes differ, no two rows or images repeat (251 is prime to every row length used here)"""
    out = []
    for H, W in sizes:
        n = H * W * C
        out.append((torch.arange(start, start + n, dtype=torch.int64) % 251).to(torch.uint8).reshape(H, W, C))
        start += n + 17
    return out


def _window_u8(images, row, h, w):
    i, y0, x0, ops = (int(v) for v in row)
    p = images[i][y0:y0 + h, x0:x0 + w]
    if ops & 1:
        p = p.flip(1)
    if ops & 2:
        p = p.flip(0)
    if ops & 4:
        p = p.transpose(0, 1)
    return p


def _ref_patch(images, row, h, w, mean=0.5, std=0.5):
    t = _window_u8(images, row, h, w).permute(2, 0, 1).float() / 255
    return (t - mean) / std


def _ref_batch(images, draws, h, w):
    return torch.stack([_ref_patch(images, r, h, w) for r in np.asarray(draws).tolist()])


def _table(images, h, w):
    """all operations valid for the window x both corner offsets x every image"""
    n_ops = 8 if h == w else 4
    return [(i, y0, x0, ops) for ops in range(n_ops) for i, im in enumerate(images)
            for (y0, x0) in ((0, 0), (im.shape[0] - h, im.shape[1] - w))]


# window -> the images of SIZES that hold it (the store of the case is those records of ONE buffer's table)
WINDOWS = (((4, 4), [0, 1, 2, 3, 4]), ((1, 1), [0, 1, 2, 3, 4]), ((33, 33), [2, 3, 4]), ((67, 65), [3, 4]), ((70, 70), [3]))


@pytest.mark.parametrize('kind', [0, 1])
@pytest.mark.parametrize('C', [1, 3, 4])
def test_gather_values(C, kind):
    """kind 0: the fp32 destination; kind 1: the uint8 destination behind resize=.  (70, 70) on the 70 x 70 image and (4, 4) on the
    4 x 4 one are windows of exactly the image's size"""
    P = pkg('patches')
    images = _images(SIZES, C)
    whole = P.PackedImages.from_images(images, 'cuda')
    assert len(whole) == 5 and whole.C == C and whole.sizes.tolist() == [list(s) for s in SIZES]
    assert (whole.table_host['offset'] % 16 == 0).all() and whole.data.dtype == torch.uint8 and whole.data.dim() == 1
    pipe = P.PatchPipeline(RESIZE, (1, 1))
    for (h, w), held in WINDOWS:
        store = whole if len(held) == 5 else P.PackedImages.from_packed(whole.data, whole.table_host[held], C=C)
        imgs = [images[i] for i in held]
        src = P.RaggedPatchSource(store, 1, (1, 1), crop=(h, w), resize=RESIZE if kind == 1 else None)
        table = _table(imgs, h, w)
        got = src.gather(np.array(table, dtype=np.int64))
        if kind == 0:
            assert got.dtype == torch.float32 and tuple(got.shape) == (len(table), C, h, w)
            got = got.cpu()
            for k, row in enumerate(table):
                assert torch.equal(got[k], _ref_patch(imgs, row, h, w)), (C, (h, w), row)
        else:
            want = pipe.resize_normalize(torch.stack([_window_u8(imgs, row, h, w) for row in table]).cuda())
            assert tuple(got.shape) == (len(table), C) + RESIZE and torch.equal(got, want), (C, (h, w))


def test_gather_other_mean_and_std_and_bad_rows():
    P = pkg('patches')
    images = _images(SIZES, 3)
    store = P.PackedImages.from_images([im.cuda() if k % 2 else im for k, im in enumerate(images)], 'cuda')      # host and device images
    src = P.RaggedPatchSource(store, 16, (2, 2), crop=(4, 4), mean=0.4, std=0.3)
    rows = [(4, 63, 127, 7), (0, 0, 0, 0), (2, 29, 61, 5), (1, 3, 5, 2)]
    want = torch.stack([_ref_patch(images, r, 4, 4, 0.4, 0.3) for r in rows])
    for table in (torch.tensor(rows), torch.tensor(rows, dtype=torch.int32).cuda(), np.array(rows, dtype=np.int32), rows):
        assert torch.equal(src.gather(table).cpu(), want)
    # every row is held to ITS image: (1, 3, 5) is the last window of the 7 x 9 image, one further is refused
    for bad in ((5, 0, 0, 0), (-1, 0, 0, 0), (1, 4, 0, 0), (1, 0, 6, 0), (0, 1, 0, 0), (0, 0, 1, 0), (2, 30, 0, 0), (2, 0, 62, 0),
                (0, -1, 0, 0), (0, 0, 0, 8), (0, 0, 0, -1)):
        with pytest.raises(ValueError):
            src.gather([(0, 0, 0, 0), bad])
    with pytest.raises(ValueError):
        src.gather(np.zeros((3, 3), dtype=np.int64))
    with pytest.raises(ValueError):
        P.RaggedPatchSource(store, 16, (2, 2), crop=(4, 3)).gather([(0, 0, 0, 4)])                # transposition, 4 x 3 window
    with pytest.raises(ValueError, match=r'image 0 \(4 x 4\)'):
        P.RaggedPatchSource(store, 16, (2, 2), crop=(5, 5))
    with pytest.raises(RuntimeError):
        P.PackedImages.from_packed(store.data[::2], store.table_host[:2])                          # a valid table, not contiguous


def test_offsets_past_two_to_the_31():
    """one 2.1 GB buffer, only the two image regions filled: the second image starts 4096 bytes past 2^31"""
    P = pkg('patches')
    a, b = _images(((9, 7), (9, 7)), 3, start=5)
    far = 2 ** 31 + 4096
    data = torch.empty(2 ** 31 + 65536, dtype=torch.uint8, device='cuda')
    data[:a.numel()].copy_(a.reshape(-1))
    data[far:far + b.numel()].copy_(b.reshape(-1))
    store = P.PackedImages.from_packed(data, np.array([(0, 9, 7), (far, 9, 7)], dtype=np.int64))
    assert store.table_host['offset'].tolist() == [0, far]
    for (h, w), resize in (((9, 7), None), ((4, 4), None), ((5, 3), RESIZE)):
        src = P.RaggedPatchSource(store, 1, (1, 1), crop=(h, w), resize=resize)
        table = _table([a, b], h, w)
        got = src.gather(table)
        if resize is None:
            assert torch.equal(got.cpu(), _ref_batch([a, b], table, h, w)), (h, w)
        else:
            want = P.PatchPipeline(RESIZE, (1, 1)).resize_normalize(torch.stack([_window_u8([a, b], r, h, w) for r in table]).cuda())
            assert torch.equal(got, want)
    del src, store, data
    torch.cuda.empty_cache()


@pytest.mark.parametrize('resize', [None, (12, 10)])
@pytest.mark.parametrize('order', ['random', 'sequential'])
def test_equal_size_store_is_the_uniform_source(order, resize):
    P = pkg('patches')
    images = _images(((20, 24),) * 40, 3)
    kw = dict(crop=(8, 8), resize=resize, hflip=True, vflip=True, transpose=True, order=order, seed=5)
    uniform = P.DevicePatchSource(torch.stack(images).cuda(), 16, (4, 4), **kw)
    ragged = P.RaggedPatchSource(P.PackedImages.from_images(images, 'cuda'), 16, (4, 4), **kw)
    assert uniform.epoch_length == ragged.epoch_length == 2
    for t in range(5):
        (hr_u, lr_u), (hr_r, lr_r) = uniform(), ragged()
        assert torch.equal(uniform.last_draws, ragged.last_draws), (order, t)
        assert torch.equal(hr_u, hr_r) and torch.equal(lr_u, lr_r), (order, t)
    assert int(uniform.step_count) == int(ragged.step_count) == 5


M37 = tuple(SIZES[i % 5] for i in range(37))


@pytest.mark.parametrize('order', ['random', 'sequential', 'permuted'])
def test_draws_match_the_host_restatement_on_a_ragged_store(order):
    """B 4, world 2: nb = 4; 3 nb + 1 steps on both ranks"""
    P = pkg('patches')
    images = _images(M37, 3)
    store = P.PackedImages.from_images(images, 'cuda')
    per_epoch = {}
    for rank in range(2):
        src = P.RaggedPatchSource(store, 4, (2, 2), crop=(4, 4), hflip=True, vflip=True, transpose=True, order=order, seed=11,
                                  rank=rank, world=2)
        assert src.epoch_length == 4 and int(src.step_count) == 0
        for t in range(13):
            img_hr, img_lr = src()
            want = P.expected_draws(11, t, 4, 37, 0, 0, 4, 4, 7, order, rank, 2, sizes=store.sizes)
            assert np.array_equal(src.last_draws.cpu().numpy(), want), (order, rank, t)
            assert int(src.step_count) == t + 1
            assert torch.equal(img_hr.cpu(), _ref_batch(images, want, 4, 4)) and tuple(img_lr.shape) == (4, 3, 2, 2)
            per_epoch.setdefault(t // 4, []).extend(want[:, 0].tolist())
    if order == 'permuted':
        for e in range(3):
            assert len(per_epoch[e]) == len(set(per_epoch[e])) == 32                               # both ranks: disjoint images


def test_permuted_order_on_the_uniform_source():
    P = pkg('patches')
    images = _images(((7, 9),) * 37, 3)
    src = P.DevicePatchSource(torch.stack(images).cuda(), 8, (2, 2), crop=(4, 4), hflip=True, order='permuted', seed=3)
    assert src.epoch_length == 4
    for e in range(2):
        seen = []
        for k in range(4):
            img_hr, _ = src()
            want = P.expected_draws(3, 4 * e + k, 8, 37, 7, 9, 4, 4, 1, 'permuted')
            assert np.array_equal(src.last_draws.cpu().numpy(), want)
            assert torch.equal(img_hr.cpu(), _ref_batch(images, want, 4, 4))
            seen += want[:, 0].tolist()
        assert len(set(seen)) == 32


def test_captured_permuted_source_crosses_epochs():
    """M 37, B 8: nb = 4.  The two warm-ups of GraphedStep drew steps 0 and 1; eleven replays draw steps 2 .. 12: the rest of
    epoch 0, epochs 1 and 2 whole, the first batch of epoch 3"""
    P, G, U = pkg('patches'), pkg('graph'), pkg('utils')
    images = _images(M37, 3)
    src = P.RaggedPatchSource(P.PackedImages.from_images(images, 'cuda'), 8, (2, 2), crop=(4, 4), hflip=True, vflip=True,
                              transpose=True, order='permuted', seed=5)
    calls = [0]

    def draw():
        calls[0] += 1
        return src()
    step = G.GraphedStep(draw)
    warm = int(src.step_count)
    assert warm == calls[0] - 1                      # every call but the captured one ran
    epochs = {}
    for k in range(11):
        t = int(src.step_count)
        assert t == warm + k
        img_hr, img_lr = step()
        assert int(src.step_count) == t + 1
        draws = src.last_draws.cpu().numpy()
        assert np.array_equal(draws, P.expected_draws(5, t, 8, 37, 0, 0, 4, 4, 7, 'permuted', sizes=src.packed.sizes)), t
        assert torch.equal(img_hr.cpu(), _ref_batch(images, draws, 4, 4)), t
        assert torch.equal(img_lr, U.lr_from_hr(img_hr, (2, 2)))
        epochs.setdefault(t // 4, []).extend(draws[:, 0].tolist())
    whole = [e for e, seen in epochs.items() if len(seen) == 32]
    assert len(epochs) >= 3 and len(whole) >= 2
    for e in whole:
        assert len(set(epochs[e])) == 32, e
    assert epochs[whole[0]] != epochs[whole[1]]      # a new order every epoch


def test_kernel_clamps_a_table_that_is_out_of_range():
    """through the C ABI (gather() validates on the host first): whatever the draw table holds, the kernel reads inside the drawn
    image and writes inside the destination -- the values are those of the clamped row, the guards stay intact"""
    from gpu_helpers import Buf, run2
    P, L = pkg('patches'), pkg('_lib')
    images = _images(SIZES, 3)
    store = P.PackedImages.from_images(images, 'cuda')
    h, w = 4, 3
    rows = [(9, -3, 1000, 7), (-2, 99, -1, 4 | 8 | 2), (2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1, -1), (1, 4, 7, 1), (2, 30, 5, 0), (0, 1, 2, 0)]
    clamped = [(4, 0, 128, 3), (0, 0, 0, 2), (4, 0, 128, 3), (1, 3, 6, 1), (2, 29, 5, 0), (0, 0, 1, 0)]      # bit 2 ignored: 4 x 3
    table = torch.tensor(rows, dtype=torch.int32).cuda()
    out = Buf(len(rows) * 3 * h * w)
    run2(lambda: L.lib().sisr_patch_gather_table(store.data.data_ptr(), store.data.numel(), store.table.data_ptr(), 5, 3,
                                                 table.data_ptr(), len(rows), h, w, 0.5, 0.5, out.ptr(), 0,
                                                 torch.cuda.current_stream().cuda_stream), [out])
    assert torch.equal(out.cpu().reshape(len(rows), 3, h, w), _ref_batch(images, clamped, h, w))


def test_resume_mid_epoch_from_a_state_dict():
    P = pkg('patches')
    images = _images(M37, 3)
    store = P.PackedImages.from_images(images, 'cuda')
    kw = dict(crop=(4, 4), hflip=True, vflip=True, transpose=True, order='permuted')
    src = P.RaggedPatchSource(store, 8, (2, 2), seed=5, **kw)
    for _ in range(6):                                # epoch 1, two of its four batches drawn
        src()
    state = src.state_dict()
    assert int(state['step_count']) == 6 and state['seed'] == 5 and state['order'] == 'permuted'
    nxt = [tuple(t.clone() for t in src()) for _ in range(3)]                 # the rest of epoch 1, the first batch of epoch 2
    assert int(state['step_count']) == 6             # a snapshot, not the live count
    fresh = P.RaggedPatchSource(store, 8, (2, 2), seed=999, **dict(kw, order='random'))
    count = fresh.step_count
    fresh.load_state_dict(state)
    assert fresh.step_count is count and int(count) == 6 and fresh.seed == 5 and fresh.order == 'permuted'
    for hr, lr in nxt:
        got_hr, got_lr = fresh()
        assert torch.equal(got_hr, hr) and torch.equal(got_lr, lr)
    want = P.expected_draws(5, 8, 8, 37, 0, 0, 4, 4, 7, 'permuted', sizes=store.sizes)
    assert np.array_equal(fresh.last_draws.cpu().numpy(), want) and torch.equal(nxt[2][0].cpu(), _ref_batch(images, want, 4, 4))
    with pytest.raises(ValueError):
        fresh.load_state_dict(dict(state, world=5))                          # 37 < 8 * 5: no batch in a permuted epoch
