"""GPU: the device-resident patch source (patches.DevicePatchSource, csrc/patchsrc.hip).

The reference throughout is torch on the CPU, written here: slice the window, flip(1) for bit 0, flip(0) for bit 1,
transpose(0, 1) for bit 2, permute to CHW, ``.float() / 255``, ``(t - mean) / std``.  Kernel and reference perform the same two
correctly rounded fp32 operations on the same 8-bit value, so the bound is bit-equality (torch.equal).

The gather kernel's tile is 32 x 32 window pixels (PG_T in csrc/patchsrc.hip): the 70 x 70 and 67 x 131 windows below span
3 x 3 and 3 x 5 tiles with ragged remainders of 6, 3 and 3 pixels."""
import os

import numpy as np
import pytest
import torch

from gpu_helpers import pkg

pytestmark = pytest.mark.gpu


def _dataset(shape):
    """arange-like: neighbouring bytes differ and no two rows or images repeat (251 is prime to every row length used here)"""
    return (torch.arange(int(np.prod(shape)), dtype=torch.int64) % 251).to(torch.uint8).reshape(shape)


def _ref_patch(data, row, h, w, mean=0.5, std=0.5):
    i, y0, x0, ops = (int(v) for v in row)
    p = data[i, y0:y0 + h, x0:x0 + w]
    if ops & 1:
        p = p.flip(1)
    if ops & 2:
        p = p.flip(0)
    if ops & 4:
        p = p.transpose(0, 1)
    t = p.permute(2, 0, 1).float() / 255
    return (t - mean) / std


def _ref_batch(data, draws, h, w, mean=0.5, std=0.5):
    return torch.stack([_ref_patch(data, r, h, w, mean, std) for r in np.asarray(draws).tolist()])


def _table(M, H0, W0, h, w):
    """all operations valid for the window x both corner offsets x first and last image"""
    n_ops = 8 if h == w else 4
    return [(i, y0, x0, ops) for ops in range(n_ops) for (y0, x0) in ((0, 0), (H0 - h, W0 - w)) for i in (0, M - 1)]


SMALL_WINDOWS = ((7, 9), (4, 4), (1, 1), (5, 3))
BIG_WINDOWS = ((70, 70), (67, 131))


def _check_gather(data, windows, kind, mean=0.5, std=0.5):
    P = pkg('patches')
    dev = data.cuda()
    M, H0, W0, C = data.shape
    for h, w in windows:
        src = P.DevicePatchSource(dev, 1, (1, 1), crop=(h, w), resize=(h, w) if kind == 1 else None, mean=mean, std=std)
        table = _table(M, H0, W0, h, w)
        got = src.gather(np.array(table, dtype=np.int64))
        assert got.dtype == torch.float32 and tuple(got.shape) == (len(table), C, h, w)
        got = got.cpu()
        for k, row in enumerate(table):
            assert torch.equal(got[k], _ref_patch(data, row, h, w, mean, std)), (C, (h, w), kind, row)


@pytest.mark.parametrize('kind', [0, 1])
@pytest.mark.parametrize('C', [1, 3, 4])
def test_gather_values_small(C, kind):
    """kind 0: the fp32 destination; kind 1: the uint8 destination, reached through resize= equal to the window (both resize
    passes are skipped, the existing kernel only normalises)"""
    _check_gather(_dataset((5, 7, 9, C)), SMALL_WINDOWS, kind)


@pytest.mark.parametrize('kind', [0, 1])
def test_gather_values_across_tiles(kind):
    _check_gather(_dataset((3, 80, 150, 3)), BIG_WINDOWS, kind)


@pytest.mark.parametrize('kind', [0, 1])
def test_gather_values_other_mean_and_std(kind):
    _check_gather(_dataset((5, 7, 9, 3)), ((4, 4), (5, 3)), kind, mean=0.4, std=0.3)


def test_gather_accepts_tensors_and_refuses_bad_rows():
    P = pkg('patches')
    data = _dataset((5, 7, 9, 3))
    src = P.DevicePatchSource(data.cuda(), 16, (2, 2), crop=(4, 4))
    rows = [(4, 3, 5, 7), (0, 0, 0, 0), (2, 1, 2, 5)]
    want = _ref_batch(data, rows, 4, 4)
    for table in (torch.tensor(rows), torch.tensor(rows, dtype=torch.int32).cuda(), np.array(rows, dtype=np.int32), rows):
        assert torch.equal(src.gather(table).cpu(), want)
    for bad in ((5, 0, 0, 0), (-1, 0, 0, 0), (0, 4, 0, 0), (0, 0, 6, 0), (0, -1, 0, 0), (0, 0, 0, 8), (0, 0, 0, -1)):
        with pytest.raises(ValueError):
            src.gather([(0, 0, 0, 0), bad])
    with pytest.raises(ValueError):
        src.gather(np.zeros((3, 3), dtype=np.int64))
    with pytest.raises(ValueError):
        src.gather(np.zeros((3, 4), dtype=np.float32))
    with pytest.raises(ValueError):
        P.DevicePatchSource(data.cuda(), 16, (2, 2), crop=(5, 3)).gather([(0, 0, 0, 4)])          # transposition, 5 x 3 window
    with pytest.raises(RuntimeError):
        P.DevicePatchSource(data.cuda().permute(0, 2, 1, 3), 16, (2, 2), crop=(4, 4))             # not contiguous


def test_kernel_clamps_a_table_that_is_out_of_range():
    """through the C ABI (gather() validates on the host first): whatever the table holds, the kernel reads inside the dataset and
    writes inside the destination -- the values are those of the clamped row, the guards stay intact"""
    from gpu_helpers import Buf, run2
    L = pkg('_lib')
    data = _dataset((5, 7, 9, 3))
    dev = data.cuda()
    h, w = 5, 3
    rows = [(9, -3, 1000, 7), (-2, 99, -1, 4 | 8 | 2), (2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1, -1)]
    clamped = [(4, 0, 6, 3), (0, 2, 0, 2), (4, 0, 6, 3)]            # bit 2 is ignored for a non-square window
    table = torch.tensor(rows, dtype=torch.int32).cuda()
    out = Buf(len(rows) * 3 * h * w)
    run2(lambda: L.lib().sisr_patch_gather(dev.data_ptr(), 5, 7, 9, 3, table.data_ptr(), len(rows), h, w, 0.5, 0.5, out.ptr(), 0,
                                           torch.cuda.current_stream().cuda_stream), [out])
    assert torch.equal(out.cpu().reshape(len(rows), 3, h, w), _ref_batch(data, clamped, h, w))


@pytest.mark.parametrize('order', ['random', 'sequential'])
def test_draws_match_the_host_restatement(order):
    """B 16 on the (5, 7, 9, 3) dataset in random order.  Sequential order has no full batch of 16 among 5 images (refused,
    asserted below), so it runs at B 16 on 40 images of the same size and at B 2 on the 5"""
    P = pkg('patches')
    cases = [((5, 7, 9, 3), 16)] if order == 'random' else [((40, 7, 9, 3), 16), ((5, 7, 9, 3), 2)]
    if order == 'sequential':
        with pytest.raises(ValueError):
            P.DevicePatchSource(_dataset((5, 7, 9, 3)).cuda(), 16, (2, 2), crop=(4, 4), order=order)
    for shape, B in cases:
        data = _dataset(shape)
        src = P.DevicePatchSource(data.cuda(), B, (2, 2), crop=(4, 4), hflip=True, vflip=True, transpose=True, order=order, seed=11)
        assert src.step_count.dtype == torch.int64 and src.step_count.dim() == 0 and int(src.step_count) == 0
        assert src.last_draws.dtype == torch.int32 and tuple(src.last_draws.shape) == (B, 4)
        for t in range(4):
            img_hr, _ = src()
            want = P.expected_draws(11, t, B, shape[0], 7, 9, 4, 4, 7, order)
            assert np.array_equal(src.last_draws.cpu().numpy(), want), (order, t)
            assert int(src.step_count) == t + 1
            assert torch.equal(img_hr.cpu(), _ref_batch(data, want, 4, 4))


def test_reference_input_side_matches_the_golden_pipeline(golden_dir):
    """crop=None, resize=image_size_hr, order='sequential', no operation: config.py:225-251 + train.py:45-46"""
    P = pkg('patches')
    z = np.load(os.path.join(golden_dir, 'patch_pipeline.npz'))
    for i in range(int(z['n'])):
        imgs = torch.from_numpy(z['imgs%d' % i])
        hr, lr = tuple(int(v) for v in z['hr_size%d' % i]), tuple(int(v) for v in z['lr_size%d' % i])
        src = P.DevicePatchSource(imgs.cuda(), imgs.shape[0], lr, crop=None, resize=hr, order='sequential')
        img_hr, img_lr = src()
        assert src.last_draws.cpu().tolist() == [[k, 0, 0, 0] for k in range(imgs.shape[0])]
        assert torch.equal(img_hr.cpu(), torch.from_numpy(z['img_hr%d' % i])), i
        assert float((img_lr.cpu() - torch.from_numpy(z['img_lr%d' % i])).abs().max()) < 1e-5, i


E2E = dict(shape=(5, 20, 24, 3), B=16, crop=(8, 8), lr=(4, 4), seed=5)


def _e2e_source(data):
    P = pkg('patches')
    return P.DevicePatchSource(data.cuda(), E2E['B'], E2E['lr'], crop=E2E['crop'], hflip=True, vflip=True, transpose=True,
                               seed=E2E['seed'])


def _e2e_ref(data, t):
    P = pkg('patches')
    M, H0, W0, _ = data.shape
    h, w = E2E['crop']
    return _ref_batch(data, P.expected_draws(E2E['seed'], t, E2E['B'], M, H0, W0, h, w, 7), h, w)


def test_end_to_end_batch():
    U = pkg('utils')
    data = _dataset(E2E['shape'])
    src = _e2e_source(data)
    img_hr, img_lr = src()
    assert tuple(img_hr.shape) == (16, 3, 8, 8) and tuple(img_lr.shape) == (16, 3, 4, 4)
    assert torch.equal(img_hr.cpu(), _e2e_ref(data, 0))
    assert torch.equal(img_lr, U.lr_from_hr(img_hr, (4, 4)))


def test_captured_source_advances_on_every_replay():
    G, U = pkg('graph'), pkg('utils')
    data = _dataset(E2E['shape'])
    src = _e2e_source(data)
    step = G.GraphedStep(lambda: src())
    batches = []
    for _ in range(3):
        t = int(src.step_count)                      # the warm-ups advanced the count, the capture itself ran nothing
        img_hr, img_lr = step()
        assert int(src.step_count) == t + 1
        assert torch.equal(img_hr.cpu(), _e2e_ref(data, t))
        assert torch.equal(img_lr, U.lr_from_hr(img_hr, (4, 4)))
        batches.append(img_hr.clone())
    assert not torch.equal(batches[0], batches[1]) and not torch.equal(batches[1], batches[2]) and not torch.equal(batches[0], batches[2])


def test_resume_from_a_state_dict():
    data = _dataset(E2E['shape'])
    src = _e2e_source(data)
    for _ in range(2):
        src()
    state = src.state_dict()
    assert int(state['step_count']) == 2 and state['seed'] == E2E['seed'] and state['order'] == 'random'
    assert (state['rank'], state['world']) == (0, 1)
    nxt = [tuple(t.clone() for t in src()) for _ in range(2)]
    assert int(state['step_count']) == 2              # a snapshot, not the live count
    P = pkg('patches')
    fresh = P.DevicePatchSource(data.cuda(), E2E['B'], E2E['lr'], crop=E2E['crop'], hflip=True, vflip=True, transpose=True, seed=999)
    count = fresh.step_count
    fresh.load_state_dict(state)
    assert fresh.step_count is count and int(count) == 2 and fresh.seed == E2E['seed']
    for hr, lr in nxt:
        got_hr, got_lr = fresh()
        assert torch.equal(got_hr, hr) and torch.equal(got_lr, lr)
    assert torch.equal(nxt[1][0].cpu(), _e2e_ref(data, 3))
