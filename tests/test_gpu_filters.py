"""GPU: the separable Gaussian filter with a mirrored border (forward, backward) and the unsharp mask on it (csrc/gauss.hip,
filters.py) against the float64 restatements of filters_cases.py, through the C entry points (guards around
every output) and through the Python surface.

Bounds.  Blur, forward and backward: 2e-6 absolute -- torch's own fp32 composition (reflect F.pad + conv2d) is 1.0e-8 .. 2.5e-7 from
float64 on these cases on a CPU, the kernels sum in another order, so 8 x the largest of those; the rigorous bound for 102 terms
of magnitude <= 1.2 is 102 x 2^-24 x 1.2 = 7e-6.  USM output: 5e-6 -- a blur error on res times weight (1e-6), a blur error on soft
times |sharp - x| <= 0.5 x 2.4 (2.4e-6), and the roundings of the last two lines.  The mask is compared element by element: it may
differ from the restatement's only where the restated level |res| 255 / (hi - lo) lies within NEAR = 5.1e-4 of the threshold
(2 x the blur bound x 127.5), and the output is then compared with the restatement run on the DEVICE's mask, so no element is left
out.  The adjoint identity <blur(x), g> = <x, blur^T(g)>, both sides summed in float64 from the device's fp32 outputs, is held to
1e-5 of the larger of the two sides, with x and g zero-mean noise: the products are cancelling sums, the hardest inputs for it."""
import numpy as np
import pytest
import torch

from filters_cases import BLUR_BOUND, CASES, F64, NEAR, NEAR_SHARE, USM_BOUND, blur64, blur64_T, blur_case, natural, noise, pkg, usm64, usm_case
from gpu_helpers import Buf, run2

pytestmark = pytest.mark.gpu
IDS = [str(c).replace(' ', '') for c in CASES]
BIG = ((1, 3, 40, 70), 51)                       # H > 25: a plane the 51-tap USM takes, two tile rows and two tile columns


def _taps(K):
    return torch.from_numpy(pkg('filters').gaussian_taps(K)).cuda()


def _entry(name, x, taps, out, K):
    n, c, h, w = x.shape
    fn = getattr(pkg('_lib').lib(), name)
    return lambda: fn(x.data_ptr(), taps.data_ptr(), out.ptr(), n * c, h, w, K, torch.cuda.current_stream().cuda_stream)


def _blur_entry(name, x, K):
    """-> the output of entry point `name` on the device tensor x, launched twice: status 0, guards intact, identical bits"""
    out = Buf(x.numel())
    run2(_entry(name, x, _taps(K), out, K), [out])
    return out.body.view(x.shape).clone()


@pytest.mark.parametrize('kind', ['natural', 'noise'])
@pytest.mark.parametrize('shape,K', CASES, ids=IDS)
def test_blur_forward_matches_float64(shape, K, kind):
    x, ref, _, _ = blur_case(shape, K, kind)
    y = _blur_entry('sisr_gauss_blur_fwd', x.cuda(), K)
    err = float((y.cpu().to(F64) - ref).abs().max())
    print('blur fwd %s K %d %s: max abs err %.3e (bound %.1e)' % (shape, K, kind, err, BLUR_BOUND))
    assert err <= BLUR_BOUND


def test_constant_image_and_one_tap():
    Fm = pkg('filters')
    c = torch.full((1, 2, 40, 70), 0.7317, device='cuda')
    for K in (5, 51, 63):
        err = float((Fm.gaussian_blur(c, K) - 0.7317).abs().max())
        print('constant image K %d: max |y - c| %.3e' % (K, err))
        assert err <= 1e-6
    x = noise((2, 3, 7, 5), 3).cuda()
    assert torch.equal(_blur_entry('sisr_gauss_blur_fwd', x, 1), x)              # K = 1: the identity, bit for bit
    assert torch.equal(_blur_entry('sisr_gauss_blur_bwd', x, 1), x)


@pytest.mark.parametrize('shape,K', CASES, ids=IDS)
def test_blur_backward_is_the_transpose(shape, K):
    x, _, g, ref_t = blur_case(shape, K, 'noise')
    dx = _blur_entry('sisr_gauss_blur_bwd', g.cuda(), K)                          # the second launch is bit-equal (run2)
    err = float((dx.cpu().to(F64) - ref_t).abs().max())
    y = _blur_entry('sisr_gauss_blur_fwd', x.cuda(), K).cpu().to(F64)
    lhs, rhs = float((y * g.to(F64)).sum()), float((x.to(F64) * dx.cpu().to(F64)).sum())
    scale = max(abs(lhs), abs(rhs))
    print('blur bwd %s K %d: max abs err %.3e (bound %.1e); <Gx, g> %.9e, <x, G^T g> %.9e, relative difference %.3e (bound 1e-5)'
          % (shape, K, err, BLUR_BOUND, lhs, rhs, abs(lhs - rhs) / scale))
    assert err <= BLUR_BOUND
    assert abs(lhs - rhs) <= 1e-5 * scale


def test_backward_with_asymmetric_taps():
    """the entry points take any taps: the transpose flips them, which a Gaussian cannot show"""
    K, shape = 5, (1, 2, 37, 70)
    t = np.array([0.1, 0.2, 0.3, 0.15, 0.25], np.float32)
    taps = torch.from_numpy(t).cuda()
    x, g = noise(shape, 5), noise(shape, 6)
    for name, src, ref in (('sisr_gauss_blur_fwd', x, blur64(x, t)), ('sisr_gauss_blur_bwd', g, blur64_T(g, t))):
        out, dev = Buf(src.numel()), src.cuda()
        run2(_entry(name, dev, taps, out, K), [out])
        err = float((out.cpu().view(shape).to(F64) - ref).abs().max())
        print('%s with asymmetric taps: max abs err %.3e' % (name, err))
        assert err <= BLUR_BOUND


@pytest.mark.parametrize('shape,K,pixel', [((1, 1, 37, 70), 5, (1, 2)), ((1, 1, 37, 70), 5, (20, 66)), ((1, 1, 40, 33), 21, (38, 1)),
                                           ((1, 1, 70, 131), 51, (33, 64))])
def test_a_non_finite_value_stays_inside_the_filters_support(shape, K, pixel):
    """one NaN pixel: the outputs that are NaN are exactly those the float64 restatement gives a non-zero weight from that pixel
    (every tap is positive) -- no term is multiplied by a zero weight, in the sliding tap window or in the border folds"""
    taps = pkg('filters').gaussian_taps(K).astype(np.float64)
    one = torch.zeros(shape, dtype=F64)
    one[0, 0, pixel[0], pixel[1]] = 1.0
    x = noise(shape, 7)
    x[0, 0, pixel[0], pixel[1]] = float('nan')
    for name, reach in (('sisr_gauss_blur_fwd', blur64(one, taps) > 0), ('sisr_gauss_blur_bwd', blur64_T(one, taps) > 0)):
        got = torch.isnan(_blur_entry(name, x.cuda(), K)).cpu()
        print('%s %s K %d NaN at %s: %d outputs NaN, %d expected' % (name, shape, K, pixel, int(got.sum()), int(reach.sum())))
        assert torch.equal(got, reach)


@pytest.mark.parametrize('shape,K', [CASES[1], CASES[3], CASES[4]], ids=[IDS[1], IDS[3], IDS[4]])
def test_autograd_function_is_the_two_entry_points(shape, K):
    Fm = pkg('filters')
    x, _, g, _ = blur_case(shape, K, 'noise')
    xd, gd = x.cuda().requires_grad_(), g.cuda()
    y = Fm.gaussian_blur(xd, K)
    assert y.requires_grad
    gx, = torch.autograd.grad(y, xd, gd)
    assert torch.equal(y.detach(), _blur_entry('sisr_gauss_blur_fwd', x.cuda(), K))
    assert torch.equal(gx, _blur_entry('sisr_gauss_blur_bwd', gd, K))
    assert torch.equal(pkg().gaussian_blur(x.cuda(), K, 0.0), y.detach())


@pytest.mark.parametrize('amp', [0.04, 0.08])
@pytest.mark.parametrize('shape,K', CASES, ids=IDS)
def test_usm_matches_float64_element_by_element(shape, K, amp):
    Fm = pkg('filters')
    x, _, mask64, level = usm_case(shape, K, amp)
    y, mask = Fm.usm_sharpen(x.cuda(), 0.5, K, 10.0, return_mask=True)
    y, mask = y.cpu(), mask.cpu()
    assert mask.dtype == torch.uint8 and int(mask.max()) <= 1
    near = (level - 10.0).abs() <= NEAR
    differs = mask.to(F64) != mask64
    share = float(near.to(F64).mean())
    assert share <= NEAR_SHARE                                     # the condition of the comparison, asserted
    assert not bool((differs & ~near).any()), 'a mask element differs away from the threshold'
    ref = usm64(x, Fm.gaussian_taps(K).astype(np.float64), mask=mask)[0]
    err = float((y.to(F64) - ref).abs().max())
    print('usm %s K %d amp %g: mask fraction %.3f, %d of %d mask elements differ (all near ties; near-tie share %.2e), max abs err %.3e '
          '(bound %.1e)' % (shape, K, amp, float(mask.float().mean()), int(differs.sum()), mask.numel(), share, err, USM_BOUND))
    assert err <= USM_BOUND


def test_usm_entry_point_keeps_inside_its_buffers():
    """y between fp32 guards, the mask and the workspace between byte guards, launched twice"""
    shape, K = (2, 3, 7, 5), 5
    n = 2 * 3 * 7 * 5
    lib = pkg('_lib').lib()
    x = natural(shape, 21, 0.08).cuda()
    taps, y = _taps(K), Buf(n)
    ws_bytes = lib.sisr_usm_ws_bytes(6, 7, 5)
    assert ws_bytes == 5 * n
    ws, mask = (torch.full((64 + b + 64,), 7, dtype=torch.uint8, device='cuda') for b in (ws_bytes, n))
    call = lambda: lib.sisr_usm_fwd(x.data_ptr(), taps.data_ptr(), K, 0.5, 10.0, -1.0, 1.0, ws.data_ptr() + 64, y.ptr(),   # noqa: E731
                                    mask.data_ptr() + 64, 6, 7, 5, torch.cuda.current_stream().cuda_stream)
    run2(call, [y])
    for t, b in ((ws, ws_bytes), (mask, n)):
        assert bool((t[:64] == 7).all()) and bool((t[64 + b:] == 7).all())
    want, want_mask = pkg('filters').usm_sharpen(x, 0.5, K, 10.0, return_mask=True)
    assert torch.equal(y.body.view(shape), want) and torch.equal(mask[64:64 + n].view(shape), want_mask)
    assert torch.equal(ws[64 + 4 * n:64 + 5 * n].view(shape), want_mask)          # the workspace's own mask bytes


def test_usm_bit_exact_properties():
    Fm = pkg('filters')
    shape, K = BIG
    x = natural(shape, 31, 0.08).cuda()
    assert torch.equal(Fm.usm_sharpen(x, weight=0.0, radius=K), x)
    assert torch.equal(Fm.usm_sharpen(x, radius=K, threshold=255.5), x)
    y, mask = Fm.usm_sharpen(x, radius=K, return_mask=True)
    assert not torch.equal(y, x) and 0.1 < float(mask.float().mean()) < 0.9
    c = torch.full(shape, 0.3125, device='cuda')
    yc, mc = Fm.usm_sharpen(c, radius=K, return_mask=True)
    assert torch.equal(yc, c) and int(mc.max()) == 0
    # Real-ESRGAN's module: radius 50 becomes 51 taps, sigma 8
    assert torch.equal(Fm.USMSharp()(x), Fm.usm_sharpen(x))
    assert torch.equal(Fm.usm_sharpen(x), Fm.usm_sharpen(x, radius=51, sigma=8.0))
    assert torch.equal(Fm.USMSharp(radius=20)(x, 0.7, 5), Fm.usm_sharpen(x, 0.7, 21, 5.0))
    xr = x.clone().requires_grad_()
    out = Fm.usm_sharpen(xr)
    assert not out.requires_grad and out.grad_fn is None and torch.equal(out, Fm.usm_sharpen(x))


def test_usm_threshold_zero_sharpens_everywhere():
    Fm = pkg('filters')
    shape, K = BIG
    x = noise(shape, 32, 1.0)
    y, mask = Fm.usm_sharpen(x.cuda(), radius=K, threshold=0.0, return_mask=True)
    assert int(mask.min()) == 1
    x64 = x.to(F64)
    want = (x64 + 0.5 * (x64 - blur64(x64, Fm.gaussian_taps(K).astype(np.float64)))).clamp(-1, 1)
    err = float((y.cpu().to(F64) - want).abs().max())
    print('usm threshold 0: max |y - clip(x + w res)| %.3e (bound %.1e); clipped share %.3f' % (err, USM_BOUND, float((want.abs() == 1).double().mean())))
    assert err <= USM_BOUND


def test_usm_value_range_zero_one_is_the_mapped_image():
    Fm = pkg('filters')
    shape, K = CASES[4]
    x = usm_case(shape, K, 0.04)[0].cuda()
    x01 = (x + 1) / 2
    y, mask = Fm.usm_sharpen(x, radius=K, return_mask=True)
    y01, mask01 = Fm.usm_sharpen(x01, radius=K, value_range=(0.0, 1.0), return_mask=True)
    assert torch.equal(mask, mask01)                               # no near tie in this case (test_filters_cpu.py prints the share: 0)
    err = float((y01.cpu().to(F64) - (y.cpu().to(F64) + 1) / 2).abs().max())
    print('usm (0, 1) against the mapped (-1, 1) result: max abs err %.3e (bound %.1e)' % (err, USM_BOUND))
    assert err <= USM_BOUND


def test_usm_and_blur_are_capturable():
    """torch.cuda.graph captures usm_sharpen and gaussian_blur forward + backward; three replays on new contents of the static
    inputs are bit-equal to eager calls on those contents"""
    Fm = pkg('filters')
    shape, K = BIG
    sx, sg = torch.zeros(shape, device='cuda'), torch.zeros(shape, device='cuda')

    def run(x, g):
        xr = x.detach().requires_grad_()
        y = Fm.gaussian_blur(xr, K)
        gx, = torch.autograd.grad(y, xr, g)
        return Fm.usm_sharpen(x, radius=K), y.detach(), gx
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            run(sx, sg)                                            # warm-up: the device taps are made here, not in the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run(sx, sg)
    for rep in range(3):
        x, g = natural(shape, 40 + rep, 0.08).cuda(), noise(shape, 50 + rep).cuda()
        sx.copy_(x)
        sg.copy_(g)
        graph.replay()
        torch.cuda.synchronize()
        eager = run(x, g)
        assert all(torch.equal(a, b) for a, b in zip(out, eager)), rep
        assert not torch.equal(out[0], x)
