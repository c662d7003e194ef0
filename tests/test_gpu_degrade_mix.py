"""GPU: the second-order degradation (degrade.py, csrc/degrade.hip): the mixed draw against its host
restatement and the float64 formulas, the noise operator against a float64 restatement built from expected_noise, the composition
against the same public operators called by hand, capture, checkpoint and install()."""
import sys

import numpy as np
import pytest
import torch

from degrade_mix_cases import FAMILIES, KERNEL_BOUND, forced_stage, kernel_error, noise64, support
from gpu_helpers import pkg

pytestmark = pytest.mark.gpu

NOISE_BOUND = 5e-6            # the existing noise bound at sigma = 0.25 (test_gpu_degrade.py: 2e-5 x 0.25)
CLAMP_MARGIN = 1e-5           # elements whose restated value lies this close to +-1 are left out of a clamped comparison
MIXES = ('realistic',) + FAMILIES


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bits(t):
    return t.view(torch.int32)


def _stage(mix, K):
    D = pkg('degrade')
    kw = dict(noise=(2 / 255., 60 / 255.), shot=(0.05, 3.0))
    if mix == 'realistic':
        return D.DegradeStage(ksize=K, ksize_min=min(K, 7), blur_prob=0.8, **kw)
    return forced_stage(mix, K, 1, **kw)


# ---- draw ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', [7, 21])
@pytest.mark.parametrize('mix', MIXES)
def test_draw_matches_the_host_restatement_and_the_formulas(mix, K):
    D = pkg('degrade')
    stage, seed, rank, t0 = _stage(mix, K), 0xC0FFEE + K, 4, (1 << 32) + 6
    d = D.HighOrderDegrader(stages=(stage,), final_sinc_prob=0.8, seed=seed, rank=rank)
    t = t0
    d.load_state_dict(dict(seed=seed, rank=rank, step=t0))
    for B in (1, 5, 37):                       # one wave, a second round of the four waves, nine rounds and a ragged tail
        k, fk, p, nt, drawn = (v.cpu().numpy() for v in d.draw_mix(0, B))
        assert int(drawn) == t and int(d.step) == t + 1
        hk, hfk, hp, hnt = D.expected_mix(seed, t, B, stage, rank=rank, final_sinc_prob=0.8)
        for col in (0, 1, 7):
            assert np.array_equal(p[:, col], hp[:, col]), col
        assert np.array_equal(nt[:, [0, 1, 3]], hnt[:, [0, 1, 3]])
        assert (np.abs(p - hp) <= 1e-6 * np.abs(hp)).all() and (np.abs(nt - hnt) <= 1e-6 * np.abs(hnt)).all()
        err = kernel_error(k, p, K)
        apart = float((np.abs(k - hk) / np.abs(hk).max(axis=(1, 2), keepdims=True)).max())
        apart_f = float((np.abs(fk - hfk) / np.abs(hfk).max(axis=(1, 2), keepdims=True)).max())
        print('%s K %d B %d: device vs float64 %.3e, device vs host %.3e, final filter device vs host %.3e' % (mix, K, B, err, apart, apart_f))
        assert err <= KERNEL_BOUND and apart <= 2 * KERNEL_BOUND and apart_f <= 2 * KERNEL_BOUND
        assert (k[~support(p, K)] == 0).all()
        if mix != 'realistic':
            assert (p[:, 0] == FAMILIES.index(mix)).all()
        t += 1
    # a second launch at the same restored step: the same bits
    d.load_state_dict(dict(seed=seed, rank=rank, step=t - 1))
    again = [v.cpu().numpy() for v in d.draw_mix(0, 37)]
    assert int(again[4]) == t - 1 and int(d.step) == t
    for a, b in zip(again[:4], (k, fk, p, nt)):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))


# ---- noise operator -----------------------------------------------------------------------------------------------------------------
NOISE_SHAPES = [(1, 1, 1, 1), (3, 3, 5, 7), (2, 4, 9, 6), (2, 1, 8, 8)]
ROWS = [(0, 0, 0.0), (1, 0, 0.25), (1, 1, 0.2), (2, 0, 0.25), (2, 1, 0.15), (0, 1, 0.1)]      # mode, grey flag, amplitude


def _noise_case(shape, start):
    x = 0.9 * (2 * torch.rand(shape, generator=_gen(sum(shape) + start)) - 1)
    table = torch.tensor([ROWS[(start + b) % 6] + (0.0,) for b in range(shape[0])], dtype=torch.float32)
    return x, table


def noise_reference(shape, start, seed, t, rank):
    """x, the table, the float64 restatement of x + n, and the elements a clamped comparison keeps (no GPU involved)"""
    x, table = _noise_case(shape, start)
    ref = x.double().numpy() + noise64(x.numpy(), table.numpy(), seed, t, rank)
    keep = np.abs(np.abs(ref) - 1) > CLAMP_MARGIN
    return x, table, ref, keep


@pytest.mark.parametrize('shape', NOISE_SHAPES, ids=['x'.join(map(str, s)) for s in NOISE_SHAPES])
def test_noise_values(shape):
    D = pkg('degrade')
    seed, rank, t = 0xABCDEF0123, 3, 41
    left_out, total = 0, 0
    for start in range(6):
        x, table, ref, keep = noise_reference(shape, start, seed, t, rank)
        left_out, total = left_out + int((~keep).sum()), total + keep.size
        step = torch.tensor(t, device='cuda')
        raw = D.degrade_noise(x.cuda(), table.cuda(), step, seed, rank, clamp=False).cpu()
        err = float(np.abs(raw.double().numpy() - ref).max())
        clamped = D.degrade_noise(x.cuda(), table.cuda(), t, seed, rank, clamp=True).cpu()        # a host int is the same step
        errc = float(np.abs(clamped.double().numpy() - np.clip(ref, -1, 1))[keep].max()) if keep.any() else 0.0
        print('noise %s rows from %d: max err %.3e, clamped %.3e' % (shape, start, err, errc))
        assert err <= NOISE_BOUND and errc <= NOISE_BOUND
        assert torch.equal(clamped, raw.clamp(-1, 1))
        n = raw.double() - x.double()
        for b in range(shape[0]):
            mode, grey, _ = ROWS[(start + b) % 6]
            if mode == 0:
                assert torch.equal(raw[b], x[b])
            else:
                assert float(n[b].abs().max()) > 0
                if grey:          # one n per pixel: the channels differ by the rounding of x + n alone
                    assert float((n[b] - n[b, :1]).abs().max()) <= 2.4e-7
                elif shape[1] > 1:
                    assert float((n[b] - n[b, :1]).abs().max()) > 1e-3
    assert left_out <= 0.02 * total           # (x in [-0.9, 0.9]: the restatement leaves out none at these seeds)


def test_shot_noise_moments():
    D = pkg('degrade')
    shape, a = (16, 3, 48, 48), 2.0
    x = 0.9 * (2 * torch.rand(shape, generator=_gen(11)) - 1)
    table = torch.tensor([[2.0, 0.0, a, 0.0]] * 16)
    y = D.degrade_noise(x.cuda(), table.cuda(), 9, 5, 0, clamp=False).cpu().double()
    z = (y - x.double()) / (a / 8 * ((x.double() + 1) / 2).clamp(0, 1).sqrt())
    n = z.numel()
    mean, var = float(z.mean()), float(z.var())
    print('shot moments over %d: mean %.3e, var - 1 %.3e' % (n, mean, var - 1))
    assert n == 110592 and abs(mean) <= 1.5e-2 and abs(var - 1) <= 2.1e-2


def test_noise_backward_is_the_clamp_mask():
    D = pkg('degrade')
    shape = (3, 3, 5, 7)
    x = 1.1 * (2 * torch.rand(shape, generator=_gen(21)) - 1)           # some outputs leave [-1, 1]
    table = torch.tensor([ROWS[1] + (0.0,), ROWS[4] + (0.0,), ROWS[0] + (0.0,)])
    dy = torch.randn(shape, generator=_gen(22)).cuda()
    xg = x.cuda().requires_grad_(True)
    y = D.degrade_noise(xg, table.cuda(), 7, 1, 0, clamp=True)
    y.backward(dy)
    mask = (y > -1) & (y < 1)
    assert bool(mask.any()) and bool((~mask).any())
    assert torch.equal(_bits(xg.grad), _bits(dy * mask))
    xg.grad = None
    D.degrade_noise(xg, table.cuda(), 7, 1, 0, clamp=False).backward(dy)
    assert torch.equal(_bits(xg.grad), _bits(dy))


# ---- composition --------------------------------------------------------------------------------------------------------------------
def _by_hand(d, x):
    """the call of HighOrderDegrader restated with the public operators and the tables the call left behind"""
    D, J = pkg('degrade'), pkg('jpeg')
    for i in range(len(d.stages)):
        final = d.last_final_kernels if i == len(d.stages) - 1 else None
        x = D.degrade(x, d.last_sizes[i], d.last_kernels[i], None, clamp=False)
        x = D.degrade_noise(x, d.last_noise_table[i], d.last_drawn_step[i], d.seed, d.rank, clamp=True)
        if final is not None and d.final_order == 'sinc_jpeg':
            x = D.degrade(x, d.last_sizes[i], final, None, clamp=True)
        if d.last_tables[i] is not None:
            x = J.jpeg_roundtrip(x, d.last_tables[i], d.jpeg_subsampling, d.jpeg_grad, True)
        if final is not None and d.final_order == 'jpeg_sinc':
            x = D.degrade(x, d.last_sizes[i], final, None, clamp=True)
    return x


def _two_stages(K, **kw):
    D = pkg('degrade')
    mk = lambda blur, sg: D.DegradeStage(ksize=K, ksize_min=min(K, 7), blur_prob=blur, sigma=sg, noise=(2 / 255., 60 / 255.),      # noqa: E731
                                         shot=(0.05, 3.0), jpeg=(30, 95))
    return D.HighOrderDegrader(stages=(mk(1.0, (0.2, 3.0)), mk(0.8, (0.2, 1.5))), mid_size=(17, 13), seed=5, **kw)


@pytest.mark.parametrize('final_order', ['sinc_jpeg', 'jpeg_sinc'])
@pytest.mark.parametrize('K', [7, 21])
def test_two_stage_call_equals_the_operators_called_by_hand(K, final_order):
    U = pkg('utils')
    x = 2 * torch.rand(3, 3, 24, 20, generator=_gen(3)) - 1
    dy = torch.randn(3, 3, 12, 10, generator=_gen(4)).cuda()
    d = _two_stages(K, final_sinc_prob=0.8, final_order=final_order)
    xg = x.cuda().requires_grad_(True)
    y = d(xg, (12, 10))
    y.backward(dy)
    assert tuple(y.shape) == (3, 3, 12, 10) and int(d.step) == 2 and d.last_sizes == [(17, 13), (12, 10)]
    assert [int(t) for t in d.last_drawn_step] == [0, 1]
    assert all(tuple(q.shape) == (3,) and tuple(tb.shape) == (3, 2, 8, 8) for q, tb in zip(d.last_quality, d.last_tables))
    xh = x.cuda().requires_grad_(True)
    yh = _by_hand(d, xh)
    yh.backward(dy)
    assert torch.equal(_bits(y.detach()), _bits(yh.detach()))
    assert torch.equal(_bits(xg.grad), _bits(xh.grad)) and float(xg.grad.abs().max()) > 0
    assert float(y.detach().abs().max()) <= 1 and not torch.equal(y.detach(), U.lr_from_hr(x.cuda(), (12, 10)))


def test_one_plain_stage_is_lr_from_hr():
    D, U = pkg('degrade'), pkg('utils')
    x = (1.2 * (2 * torch.rand(2, 3, 16, 16, generator=_gen(1)) - 1)).cuda()
    d = D.HighOrderDegrader(stages=(D.DegradeStage(ksize=5, ksize_min=1, blur_prob=0.0),), final_sinc_prob=None)
    y, ref = d(x, (8, 8)), U.lr_from_hr(x, (8, 8))
    err = float((y - ref).abs().max())
    print('one plain stage vs lr_from_hr: max err %.3e' % err)
    assert err <= 4e-6 and float(ref.abs().max()) == 1.0 and d.last_final_kernels is None and int(d.step) == 1


def test_middle_size_default_and_host_drawn_scale():
    D = pkg('degrade')
    x = (2 * torch.rand(1, 3, 24, 20, generator=_gen(2)) - 1).cuda()
    d = D.HighOrderDegrader(seed=3)
    d(x, (6, 5))
    assert d.last_sizes == [(12, 10), (6, 5)]                      # the rounded geometric mean
    shapes = []
    for _ in range(2):
        d = D.HighOrderDegrader(mid_scale=(0.3, 1.2), seed=3)
        for _ in range(3):
            d(x, (6, 5))
            shapes.append(d.last_sizes[0])
        assert d.calls == 3 and int(d.step) == 6
    assert shapes[:3] == shapes[3:] and len(set(shapes)) > 1      # one seed: the same sizes; they change from call to call


# ---- capture, checkpoint, install ------------------------------------------------------------------------------------------------------
def test_captured_call_advances_on_every_replay():
    G = pkg('graph')
    x = (2 * torch.rand(2, 3, 24, 20, generator=_gen(5)) - 1).cuda()
    d, twin = _two_stages(7), _two_stages(7)
    step = G.GraphedStep(lambda: d(x, (12, 10)))
    t0 = int(d.step)                                         # the warm-ups advanced the count, the capture itself ran nothing
    assert t0 == 2 * 2
    twin.load_state_dict(dict(d.state_dict(), step=t0))
    got = [step().clone() for _ in range(3)]
    assert int(d.step) == t0 + 2 * 3
    want = [twin(x, (12, 10)) for _ in range(3)]
    for a, b in zip(got, want):
        assert torch.equal(_bits(a), _bits(b))
    assert not torch.equal(got[0], got[1]) and not torch.equal(got[1], got[2])


def test_host_drawn_middle_size_refuses_capture():
    D, G = pkg('degrade'), pkg('graph')
    x = (2 * torch.rand(1, 3, 16, 16, generator=_gen(6)) - 1).cuda()
    d = D.HighOrderDegrader(mid_scale=(0.5, 0.9), seed=1)
    with pytest.raises(G.GraphCaptureError, match='mid_scale'):
        G.GraphedStep(lambda: d(x, (8, 8)))


def test_resume_from_a_state_dict():
    x = (2 * torch.rand(1, 3, 16, 16, generator=_gen(6)) - 1).cuda()
    d = _two_stages(7)
    d(x, (8, 8))
    state = d.state_dict()
    a = [d(x, (8, 8)) for _ in range(2)]
    fresh = _two_stages(7)
    held = fresh.step
    fresh.load_state_dict(state)
    b = [fresh(x, (8, 8)) for _ in range(2)]
    assert int(state['step']) == 2 and int(fresh.step) == 6 and fresh.step is held and fresh.calls == 3
    assert all(torch.equal(_bits(u), _bits(v)) for u, v in zip(a, b)) and not torch.equal(a[0], a[1])


def test_install_routes_lr_from_hr_through_the_degrader():
    P, U = pkg(), pkg('utils')
    x = (1.2 * (2 * torch.rand(2, 3, 16, 16, generator=_gen(8)) - 1)).cuda()
    P.install()
    mod = sys.modules['utils']
    original = mod.lr_from_hr
    d = _two_stages(7)
    try:
        P.install(degradation=d)
        y = sys.modules['utils'].lr_from_hr(x, (8, 8), device='cuda')
        assert int(d.step) == 2
        assert torch.equal(_bits(y), _bits(_by_hand(d, x))) and not torch.equal(y, original(x, (8, 8)))
    finally:
        mod.lr_from_hr = original
    assert torch.equal(mod.lr_from_hr(x, (8, 8)), U._Bicubic.apply(x, (8, 8), True))
