"""GPU: the blur + noise degradation (degrade.py, csrc/degrade.hip) against float64 restatements written here:
F.pad(mode='replicate'), a per-sample F.conv2d, F.interpolate(bicubic, align_corners=True).  The kernels are ASYMMETRIC random
non-negative tables, not Gaussians: a flipped kernel or transposed axes fail every value test."""
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gpu_helpers import pkg
from test_degrade_cpu import _noise64

pytestmark = pytest.mark.gpu

VALUE_SHAPES = [((3, 3, 24, 40), (12, 20)),          # three different kernels: sample b must use kernel b
                ((2, 3, 37, 70), (17, 33)),          # ragged tiles, non-integer ratio
                ((1, 3, 64, 64), (8, 8)),            # ratio 8
                ((1, 1, 8, 8), (16, 16)),            # up-scaling
                ((1, 1, 9, 9), (1, 4))]              # output size 1, scale 0
VALUE_CASES = [(s, o, K) for s, o in VALUE_SHAPES for K in (1, 3, 7, 21)] + [((1, 1, 5, 7), (3, 2), 21)]      # image smaller than the radius
_ids = ['%s_to_%s_k%d' % ('x'.join(map(str, s)), 'x'.join(map(str, o)), K) for s, o, K in VALUE_CASES]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _kernels(n, K, g, gain=None):
    """asymmetric, non-negative, a few dominant taps; each sums to 1, or to `gain` / (0.4 sqrt(3) |k|_2) (see the backward test)"""
    k = torch.rand(n, K, K, generator=g, dtype=torch.float64) ** 3
    k = k / k.sum(dim=(1, 2), keepdim=True)
    if gain is not None:
        k = k * gain / (0.4 * 3 ** 0.5 * k.flatten(1).norm(dim=1))[:, None, None]
    return k


def _linear64(x64, k64, size):
    """blur (correlation, replicate border) and bicubic resampling in float64 on the host"""
    n, c, h, w = x64.shape
    K = k64.shape[-1]
    R = (K - 1) // 2
    xp = F.pad(x64, (R, R, R, R), mode='replicate').reshape(1, n * c, h + 2 * R, w + 2 * R)
    b = F.conv2d(xp, k64.repeat_interleave(c, dim=0)[:, None], groups=n * c).reshape(n, c, h, w)
    return F.interpolate(b, size=size, mode='bicubic', align_corners=True)


@pytest.mark.parametrize('shape,size', [((2, 3, 16, 16), (8, 8)), ((1, 1, 13, 29), (5, 11))])
def test_delta_kernel_is_lr_from_hr(shape, size):
    D, U = pkg('degrade'), pkg('utils')
    x = (1.2 * (2 * torch.rand(shape, generator=_gen(1)) - 1)).cuda()
    k = torch.zeros(shape[0], 5, 5)
    k[:, 2, 2] = 1.0
    y, ref = D.degrade(x, size, k.cuda()), U.lr_from_hr(x, size)
    err = float((y - ref).abs().max())
    print('delta kernel vs lr_from_hr: max err %.3e' % err)
    assert tuple(y.shape) == shape[:2] + size and err <= 4e-6      # 32 roundings x 2^-24 x sum |w_y| |w_x| <= 1.95
    assert float(ref.abs().max()) == 1.0                            # the clamp is in play


@pytest.mark.parametrize('shape,size,K', VALUE_CASES, ids=_ids)
def test_forward_values(shape, size, K):
    D = pkg('degrade')
    g = _gen(K * 1000 + shape[2])
    x = 2 * torch.rand(shape, generator=g) - 1
    k = _kernels(shape[0], K, g).float()
    ref = _linear64(x.double(), k.double(), size)
    y = D.degrade(x.cuda(), size, k.cuda(), clamp=False).cpu()
    bound = (K * K + 16) * 2.0 ** -23 * 2 * float(x.abs().max())       # worst-case rounding of the two sums
    err = float((y.double() - ref).abs().max())
    print('forward %s -> %s K %d: max err %.3e, bound %.3e' % (shape, size, K, err, bound))
    assert err <= bound
    yc = D.degrade(x.cuda(), size, k.cuda()).cpu()
    assert torch.equal(yc, y.clamp(-1, 1))


@pytest.mark.parametrize('shape,size,K', VALUE_CASES, ids=_ids)
def test_backward_values(shape, size, K):
    """dx against float64 autograd of the linear part applied to dy * [-1 < y_gpu < 1] (the mask is the saved output by
    definition).  The kernels carry a gain that gives the blurred image a standard deviation near 1, so that the clamp cuts"""
    D = pkg('degrade')
    for attempt in range(64):          # (tiny images under a 21 x 21 kernel give strongly correlated outputs: the first seed that has both)
        g = _gen(K * 1000 + shape[2] + 7 + 100000 * attempt)
        x = 1.2 * (2 * torch.rand(shape, generator=g) - 1)
        k = _kernels(shape[0], K, g, gain=1.0 if K > 1 else None).float()
        dy = torch.randn(shape[:2] + size, generator=g)
        x64 = x.double().requires_grad_(True)
        ref_y = _linear64(x64, k.double(), size)
        if bool((ref_y.abs() > 1).any()) and bool((ref_y.abs() < 1).any()):
            break
    assert bool((ref_y.abs() > 1).any()) and bool((ref_y.abs() < 1).any())       # the reference itself has both kinds of output
    xg = x.cuda().requires_grad_(True)
    y = D.degrade(xg, size, k.cuda())
    y.backward(dy.cuda())
    mask = ((y > -1) & (y < 1)).cpu()
    ref_y.backward(dy.double() * mask)
    scale = float(x64.grad.abs().max())
    err = float((xg.grad.cpu().double() - x64.grad).abs().max())
    print('backward %s -> %s K %d: max err / max |dx| %.3e' % (shape, size, K, err / scale))
    assert err <= 1e-3 * scale


@pytest.mark.parametrize('shape,size,K', VALUE_CASES, ids=_ids)
def test_adjoint_identity(shape, size, K):
    D = pkg('degrade')
    g = _gen(K * 1000 + shape[2] + 13)
    x = 2 * torch.rand(shape, generator=g) - 1
    k = _kernels(shape[0], K, g).float().cuda()
    dy = torch.randn(shape[:2] + size, generator=g)
    xg = x.cuda().requires_grad_(True)
    jx = D.degrade(xg, size, k, clamp=False)
    jx.backward(dy.cuda())
    lhs = float((dy.double() * jx.detach().cpu().double()).sum())
    rhs = float((xg.grad.cpu().double() * x.double()).sum())
    scale = float((dy.double().abs() * jx.detach().cpu().double().abs()).sum())
    print('adjoint %s -> %s K %d: |lhs - rhs| / sum |dy| |Jx| %.3e' % (shape, size, K, abs(lhs - rhs) / scale))
    assert abs(lhs - rhs) <= 1e-5 * scale


@pytest.mark.parametrize('shape,size', [((1, 1, 5, 9), (3, 5)), ((2, 3, 33, 17), (17, 9))])
def test_exact_operands_are_bit_equal(shape, size):
    """H = 2h - 1: the scale is exactly 2 and the cubic weights exactly (0, 1, 0, 0); kernels are integers / 1024, x integers in
    [-8, 8], dy integers in [-4, 4], no clamp: every fp32 sum is exact, so forward AND backward equal the float64 reference bit for
    bit.  One missing border-fold tap fails this."""
    D = pkg('degrade')
    assert shape[2] == 2 * size[0] - 1 and shape[3] == 2 * size[1] - 1
    g = _gen(shape[2])
    x = torch.randint(-8, 9, shape, generator=g).float()
    k = torch.randint(0, 8, (shape[0], 21, 21), generator=g).float() / 1024
    dy = torch.randint(-4, 5, shape[:2] + size, generator=g).float()
    x64 = x.double().requires_grad_(True)
    ref = _linear64(x64, k.double(), size)
    ref.backward(dy.double())
    xg = x.cuda().requires_grad_(True)
    y = D.degrade(xg, size, k.cuda(), clamp=False)
    y.backward(dy.cuda())
    assert torch.equal(y.detach().cpu().double(), ref.detach())
    assert torch.equal(xg.grad.cpu().double(), x64.grad)


def test_noise_values_and_group_tail():
    D = pkg('degrade')
    seed, rank, t = 0xABCDEF0123, 3, 41
    x = torch.zeros(1, 3, 5, 7, device='cuda')
    k = torch.zeros(1, 3, 3, device='cuda')
    k[:, 1, 1] = 1.0
    sigma = torch.tensor([0.25], device='cuda')
    y = D.degrade(x, (3, 5), k, sigma, torch.tensor(t, device='cuda'), seed, rank, clamp=False).cpu()
    assert y.numel() == 45                                                       # 11 groups and one element of a twelfth
    ref = 0.25 * _noise64(seed, t, 0, 45, rank)
    err = float(np.abs(y.double().numpy().reshape(-1) - ref).max())
    print('noise: max err %.3e' % err)
    assert err <= 2e-5 * 0.25
    assert torch.equal(D.degrade(x, (3, 5), k, sigma, t, seed, rank, clamp=False).cpu(), y)      # a host int is the same step


def test_noise_moments():
    D = pkg('degrade')
    x = torch.zeros(16, 3, 48, 48, device='cuda')
    k = torch.ones(16, 1, 1, device='cuda')
    z = D.degrade(x, (48, 48), k, torch.ones(16, device='cuda'), 9, 5, 0, clamp=False).double()
    n = z.numel()
    mean, var = float(z.mean()), float(z.var())
    print('noise moments over %d: mean %.3e, var - 1 %.3e' % (n, mean, var - 1))
    assert abs(mean) < 5 / n ** 0.5 and abs(var - 1) < 5 * (2 / n) ** 0.5


def test_draw_matches_the_host_restatement():
    D = pkg('degrade')
    d = D.Degrader(ksize=21, sigma=(0.2, 3.0), anisotropic=True, noise=(0.01, 0.1), seed=77, rank=4)
    d.load_state_dict(dict(seed=77, rank=4, step=(1 << 32) + 6))
    for t in ((1 << 32) + 6, (1 << 32) + 7):
        assert int(d.step) == t
        k, s, drawn = d.draw(5)
        assert int(drawn) == t and int(d.step) == t + 1                          # drawn_step is the step BEFORE the draw
        hk, hs, _ = D.expected_params(77, t, 5, 21, (0.2, 3.0), True, (0.01, 0.1), 4)
        err = float((np.abs(k.cpu().numpy() - hk) / hk.max(axis=(1, 2), keepdims=True)).max())
        print('draw: max err / max weight %.3e' % err)
        assert err <= 1e-6 and np.abs(s.cpu().numpy() - hs).max() <= 1e-6 * 0.1


def _degrader(**kw):
    return pkg('degrade').Degrader(ksize=7, sigma=(0.5, 2.0), noise=(0.01, 0.05), seed=5, **kw)


def test_two_calls_at_one_step_are_bit_equal():
    x = (2 * torch.rand(2, 3, 37, 70, generator=_gen(3)) - 1).cuda()
    dy = torch.randn(2, 3, 17, 33, generator=_gen(4)).cuda()
    outs = []
    for _ in range(2):
        d = _degrader()
        xg = x.clone().requires_grad_(True)
        y = d(xg, (17, 33))
        y.backward(dy)
        outs.append((y.detach(), xg.grad, d.last_kernels, d.last_noise_sigma))
    for a, b in zip(*outs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert float(outs[0][1].abs().max()) > 0


def test_captured_degrader_advances_on_every_replay():
    G = pkg('graph')
    x = (2 * torch.rand(2, 3, 24, 40, generator=_gen(5)) - 1).cuda()
    d, twin = _degrader(), _degrader()
    step = G.GraphedStep(lambda: d(x, (12, 20)))
    t0 = int(d.step)                                         # the warm-ups advanced the count, the capture itself ran nothing
    twin.load_state_dict(dict(d.state_dict(), step=t0))
    got = [step().clone() for _ in range(3)]
    assert int(d.step) == t0 + 3
    want = [twin(x, (12, 20)) for _ in range(3)]
    for a, b in zip(got, want):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert not torch.equal(got[0], got[1]) and not torch.equal(got[1], got[2])


def test_resume_from_a_state_dict():
    x = (2 * torch.rand(1, 3, 16, 16, generator=_gen(6)) - 1).cuda()
    d = _degrader()
    d(x, (8, 8))
    state = d.state_dict()
    a = [d(x, (8, 8)) for _ in range(2)]
    fresh = _degrader()
    fresh.load_state_dict(state)
    b = [fresh(x, (8, 8)) for _ in range(2)]
    assert int(state['step']) == 1 and int(fresh.step) == 3
    assert all(torch.equal(u, v) for u, v in zip(a, b)) and not torch.equal(a[0], a[1])


def test_install_routes_lr_from_hr_through_the_degrader():
    P, D, U = pkg(), pkg('degrade'), pkg('utils')
    x = (1.2 * (2 * torch.rand(2, 3, 16, 16, generator=_gen(8)) - 1)).cuda()
    P.install()
    mod = sys.modules['utils']
    original = mod.lr_from_hr
    assert torch.equal(mod.lr_from_hr(x, (8, 8)), U._Bicubic.apply(x, (8, 8), True))      # the default: today's path, bit for bit
    d = _degrader()
    try:
        P.install(degradation=d)
        y = sys.modules['utils'].lr_from_hr(x, (8, 8), device='cuda')
        assert int(d.step) == 1
        assert torch.equal(y, D.degrade(x, (8, 8), d.last_kernels, d.last_noise_sigma, d.last_drawn_step, d.seed, d.rank))
        assert not torch.equal(y, original(x, (8, 8)))
    finally:
        mod.lr_from_hr = original
    assert torch.equal(mod.lr_from_hr(x, (8, 8)), U._Bicubic.apply(x, (8, 8), True))
