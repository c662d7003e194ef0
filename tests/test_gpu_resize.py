"""GPU: the resize of DESIGN.md section 27 (csrc/resize.hip, resize.py) against torch's float64 CPU operator -- values, gradients,
exact operands, the adjoint identity, determinism, full writes, NaN propagation, the mode draw, graph capture -- and
HighOrderDegrader(resize_probs=...) against the public operators called by hand."""
import numpy as np
import pytest
import torch

from gpu_helpers import _bits, assert_within, pkg
from resize_cases import MIXED, MODES, SHAPES, bounds, case, dyadic, interp64, noise, read_sets

pytestmark = pytest.mark.gpu
F64 = torch.float64
KINDS = MODES + ('mixed',)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _mode_arg(kind, n):
    return torch.tensor(MIXED, dtype=torch.int32, device='cuda') if kind == 'mixed' else kind


# ---- values ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('size_in,size_out', SHAPES)
def test_forward_values(size_in, size_out, kind):
    """every element against float64 F.interpolate; bound (terms + 16) 2^-23 L max|x| from the float64 tap matrices"""
    R = pkg('resize')
    x, y64, _, _, _ = case(size_in, size_out, kind)
    y = R.resize(x.cuda(), size_out, _mode_arg(kind, x.shape[0]))
    assert tuple(y.shape) == tuple(y64.shape) and y.dtype == torch.float32
    bound = bounds(size_in, size_out, kind, False, float(x.abs().max())).expand_as(y64)
    assert_within(y.cpu(), y64, bound, 'resize fwd %s %s -> %s' % (kind, size_in, size_out))


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('size_in,size_out', SHAPES)
def test_backward_values(size_in, size_out, kind):
    """every element against float64 autograd of F.interpolate; the same bound with terms and L taken over columns"""
    R = pkg('resize')
    x, _, dy, dx64, _ = case(size_in, size_out, kind)
    xg = x.cuda().requires_grad_(True)
    R.resize(xg, size_out, _mode_arg(kind, x.shape[0])).backward(dy.cuda())
    bound = bounds(size_in, size_out, kind, True, float(dy.abs().max())).expand_as(dx64)
    assert_within(xg.grad.cpu(), dx64, bound, 'resize bwd %s %s -> %s' % (kind, size_in, size_out))


@pytest.mark.parametrize('size_in,size_out', [((256, 256), (16, 16)), ((16, 16), (256, 256)), ((130, 20), (9, 300))])
def test_ratio_sixteen_runs_on_halved_tiles(size_in, size_out):
    """ratio 16 per axis, down and up: the staged block of a 16 x 64 tile does not fit 64 KB, so the host halves the tile (256 -> 16
    forward: 8 x 4; 16 -> 256 backward: 4 x 4); and 14 down beside 15 up on whole tiles.  The mixed table, values and gradients,
    the usual bounds"""
    R = pkg('resize')
    x, y64, dy, dx64, _ = case(size_in, size_out, 'mixed')
    xg = x.cuda().requires_grad_(True)
    y = R.resize(xg, size_out, _mode_arg('mixed', 3))
    y.backward(dy.cuda())
    assert_within(y.detach().cpu(), y64, bounds(size_in, size_out, 'mixed', False, float(x.abs().max())).expand_as(y64),
                  'resize fwd mixed %s -> %s' % (size_in, size_out))
    assert_within(xg.grad.cpu(), dx64, bounds(size_in, size_out, 'mixed', True, float(dy.abs().max())).expand_as(dx64),
                  'resize bwd mixed %s -> %s' % (size_in, size_out))


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('size_in,size_out', [((16, 16), (8, 8)), ((8, 8), (16, 16))])
def test_exact_operands_are_bit_equal(size_in, size_out, mode):
    """integers / 1024 in [-1, 1] at ratio 2 and 1/2: the weights are dyadic, so float64 holds every sum exactly and the kernel's
    result is that value in fp32.  At ratio 2 and for area and bilinear at 1/2 the sums carry at most 21 bits and fp32 holds them
    too; bicubic at 1/2 has weights k / 256 and its second pass carries 27 bits: the kernel adds a pass in double and rounds once,
    so it is still the float64 reference, rounded"""
    R = pkg('resize')
    x = dyadic((2, 3) + size_in, 41)
    ref = interp64(x, size_out, mode)
    y = R.resize(x.cuda(), size_out, mode).cpu()
    if not (mode == 'bicubic' and size_out > size_in):
        assert torch.equal(ref.to(torch.float32).to(F64), ref)
    assert torch.equal(_bits(y), _bits(ref.to(torch.float32)))


def test_a_mode_value_outside_the_table_is_bicubic():
    R = pkg('resize')
    x = noise((3, 2, 7, 5), 42).cuda().requires_grad_(True)
    dy = noise((3, 2, 11, 4), 43).cuda()
    odd = torch.tensor([7, -1, 1 << 30], dtype=torch.int32, device='cuda')
    y = R.resize(x, (11, 4), odd)
    y.backward(dy)
    g, x.grad = x.grad, None
    ref = R.resize(x, (11, 4), 'bicubic')
    ref.backward(dy)
    assert torch.equal(_bits(y.detach()), _bits(ref.detach())) and torch.equal(_bits(g), _bits(x.grad))


# ---- structure ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('size_in,size_out', [((33, 35), (8, 9)), ((5, 7), (11, 13)), ((40, 70), (37, 67))])
def test_adjoint_identity(size_in, size_out, kind):
    """<dy, R x> = <R^T dy, x> within 1e-5 relative (sums in float64 over the fp32 results; both tensors have mean 0.5, so the
    product is far from 0)"""
    R = pkg('resize')
    n = 3 if kind == 'mixed' else 2
    x = (noise((n, 2) + size_in, 44, 0.5) + 0.5).cuda().requires_grad_(True)
    dy = (noise((n, 2) + size_out, 45, 0.5) + 0.5).cuda()
    y = R.resize(x, size_out, _mode_arg(kind, n))
    y.backward(dy)
    a, b = float((dy.double() * y.detach().double()).sum()), float((x.grad.double() * x.detach().double()).sum())
    rel = abs(a - b) / max(abs(a), abs(b))
    print('adjoint %s %s -> %s: %.9e vs %.9e, relative %.2e' % (kind, size_in, size_out, a, b, rel))
    assert abs(a) > 1 and rel <= 1e-5


def test_two_calls_are_bit_equal():
    R = pkg('resize')
    x, dy = noise((3, 2, 40, 70), 46).cuda(), noise((3, 2, 37, 67), 47).cuda()
    modes = torch.tensor(MIXED, dtype=torch.int32, device='cuda')
    got = []
    for _ in range(2):
        xg = x.clone().requires_grad_(True)
        y = R.resize(xg, (37, 67), modes)
        y.backward(dy)
        got.append((y.detach(), xg.grad))
    assert torch.equal(_bits(got[0][0]), _bits(got[1][0])) and torch.equal(_bits(got[0][1]), _bits(got[1][1]))


@pytest.mark.parametrize('size_in,size_out', [((33, 35), (8, 9)), ((3, 50), (9, 2)), ((5, 7), (11, 13)), ((70, 130), (9, 17))])
def test_every_element_is_written(size_in, size_out):
    """y and dx buffers pre-filled with NaN come back finite, through the C ABI: no zero-fill launch stands behind the gather (the
    down-scaling bilinear and bicubic leave pixels that no output reads: their gradient is a stored 0)"""
    lib = pkg('_lib').lib()
    modes = torch.tensor(MIXED, dtype=torch.int32, device='cuda')
    n, c = 3, 2
    x, dy = noise((n, c) + size_in, 48).cuda(), noise((n, c) + size_out, 49).cuda()
    y = torch.full((n, c) + size_out, float('nan'), device='cuda')
    dx = torch.full((n, c) + size_in, float('nan'), device='cuda')
    assert lib.sisr_resize_fwd(x.data_ptr(), modes.data_ptr(), y.data_ptr(), n, c, *size_in, *size_out, None) == 0
    assert lib.sisr_resize_bwd(dy.data_ptr(), modes.data_ptr(), dx.data_ptr(), n, c, *size_in, *size_out, None) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(dx).all())
    unread = [~torch.from_numpy(np.outer(read_sets(MODES[m], size_in[0], size_out[0]).any(0), read_sets(MODES[m], size_in[1], size_out[1]).any(0)))
              for m in MIXED]
    for i, u in enumerate(unread):
        assert bool((dx[i].cpu()[:, u] == 0).all())
    if size_in[0] >= 4 * size_out[0]:
        assert bool(unread[2].any())                                # the bilinear sample skips pixels at this ratio


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('size_in,size_out,at', [((7, 5), (3, 4), (3, 2)), ((5, 7), (11, 13), (0, 6)), ((33, 35), (8, 9), (16, 17))])
def test_nan_reaches_the_outputs_that_read_it_and_no_others(size_in, size_out, at, mode):
    R = pkg('resize')
    x = noise((1, 1) + size_in, 50)
    x[0, 0, at[0], at[1]] = float('nan')
    y = R.resize(x.cuda(), size_out, mode).cpu()[0, 0]
    want = np.outer(read_sets(mode, size_in[0], size_out[0])[:, at[0]], read_sets(mode, size_in[1], size_out[1])[:, at[1]])
    assert np.array_equal(torch.isnan(y).numpy(), want)
    assert torch.equal(torch.isnan(y), torch.isnan(interp64(x, size_out, mode)[0, 0]))        # ... which is what torch does


# ---- draw and capture --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B', [1, 5, 37])
def test_device_draw_is_the_host_restatement(B):
    R = pkg('resize')
    for t, seed, rank, probs in ((0, 1, 0, (1 / 3, 1 / 3, 1 / 3)), ((1 << 33) + 9, (1 << 40) + 5, 7, (0.5, 0.0, 0.5)), (3, 2, 65535, (0, 0, 1))):
        step = torch.full((), t, dtype=torch.int64, device='cuda')
        got = R.draw_resize_modes(step, seed, rank, B, probs)
        assert got.dtype == torch.int32 and int(step) == t                                      # read, not advanced
        assert np.array_equal(got.cpu().numpy(), R.expected_resize_modes(seed, t, B, probs, rank))


def test_captured_resize_follows_the_table_at_replay():
    """a captured forward + backward with a device table; the table's contents are changed in place between replays and the replay
    resamples with the new modes, bit-equal to an eager call"""
    R = pkg('resize')
    x, dy = noise((3, 2, 24, 20), 51).cuda(), noise((3, 2, 17, 13), 52).cuda()
    table = torch.tensor([2, 2, 2], dtype=torch.int32, device='cuda')

    def run(modes):
        xr = x.detach().requires_grad_()
        y = R.resize(xr, (17, 13), modes)
        gx, = torch.autograd.grad(y, xr, dy)
        return y.detach(), gx
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            run(table)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run(table)
    seen = []
    for new in ((0, 1, 2), (1, 0, 0), (2, 2, 1)):
        table.copy_(torch.tensor(new, dtype=torch.int32))
        graph.replay()
        torch.cuda.synchronize()
        eager = run(torch.tensor(new, dtype=torch.int32, device='cuda'))
        for a, b in zip(out, eager):
            assert torch.equal(_bits(a), _bits(b))
        seen.append(out[0].clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])


# ---- HighOrderDegrader(resize_probs=...) -------------------------------------------------------------------------------------------
def _stages():
    D = pkg('degrade')
    mk = lambda blur, sg: D.DegradeStage(ksize=7, ksize_min=7, blur_prob=blur, sigma=sg, noise=(2 / 255., 60 / 255.), shot=(0.05, 3.0),      # noqa: E731
                                         jpeg=(30, 95))
    return (mk(1.0, (0.2, 3.0)), mk(0.8, (0.2, 1.5)))


def _degrader(**kw):
    return pkg('degrade').HighOrderDegrader(stages=_stages(), mid_size=(17, 13), seed=5, **kw)


def _by_hand(d, x):
    """the call restated with the public operators and the tables it left behind, ``last_modes`` included"""
    D, J, R = pkg('degrade'), pkg('jpeg'), pkg('resize')
    for i in range(len(d.stages)):
        final = d.last_final_kernels if i == len(d.stages) - 1 else None
        x = D.degrade(x, tuple(x.shape[2:]), d.last_kernels[i], None, clamp=False)
        x = R.resize(x, d.last_sizes[i], d.last_modes[i])
        x = D.degrade_noise(x, d.last_noise_table[i], d.last_drawn_step[i], d.seed, d.rank, clamp=True)
        if final is not None:
            x = D.degrade(x, d.last_sizes[i], final, None, clamp=True)
        if d.last_tables[i] is not None:
            x = J.jpeg_roundtrip(x, d.last_tables[i], d.jpeg_subsampling, d.jpeg_grad, True)
    return x


def test_degrader_with_drawn_resamplers_equals_the_operators_called_by_hand():
    R = pkg('resize')
    probs = (1 / 3, 1 / 3, 1 / 3)
    x = 2 * torch.rand(3, 3, 24, 20, generator=_gen(3)) - 1
    dy = torch.randn(3, 3, 12, 10, generator=_gen(4)).cuda()
    d = _degrader(resize_probs=probs)
    xg = x.cuda().requires_grad_(True)
    y = d(xg, (12, 10))
    y.backward(dy)
    assert tuple(y.shape) == (3, 3, 12, 10) and int(d.step) == 2 and d.last_sizes == [(17, 13), (12, 10)]
    for i in range(2):                                                 # the draw is keyed by the stage's drawn step; the count did not move
        assert np.array_equal(d.last_modes[i].cpu().numpy(), R.expected_resize_modes(5, int(d.last_drawn_step[i]), 3, probs))
    xh = x.cuda().requires_grad_(True)
    yh = _by_hand(d, xh)
    yh.backward(dy)
    assert torch.equal(_bits(y.detach()), _bits(yh.detach()))
    assert torch.equal(_bits(xg.grad), _bits(xh.grad)) and float(xg.grad.abs().max()) > 0
    assert float(y.detach().abs().max()) <= 1
    assert sorted(d.state_dict()) == sorted(_degrader().state_dict())  # no new field


def test_degrader_with_drawn_resamplers_is_capturable():
    G = pkg('graph')
    x = (2 * torch.rand(3, 3, 24, 20, generator=_gen(5)) - 1).cuda()
    probs = (1 / 3, 1 / 3, 1 / 3)
    d, twin = _degrader(resize_probs=probs), _degrader(resize_probs=probs)
    step = G.GraphedStep(lambda: d(x, (12, 10)))
    t0 = int(d.step)
    twin.load_state_dict(dict(d.state_dict(), step=t0))
    got = [step().clone() for _ in range(3)]
    want = [twin(x, (12, 10)) for _ in range(3)]
    assert int(d.step) == t0 + 2 * 3
    for a, b in zip(got, want):
        assert torch.equal(_bits(a), _bits(b))
    assert not torch.equal(got[0], got[1]) and not torch.equal(got[1], got[2])


def test_degrader_without_resize_probs_is_unchanged(monkeypatch):
    """resize_probs=None: no sisr_resize_* call, and the bits of an instance built without the keyword"""
    lib = pkg('_lib').lib()

    def refuse(*args):
        raise AssertionError('a resize entry point was called')
    for name in ('sisr_resize_fwd', 'sisr_resize_bwd', 'sisr_resize_modes_draw'):
        monkeypatch.setattr(lib, name, refuse)
    x = 2 * torch.rand(3, 3, 24, 20, generator=_gen(6)) - 1
    dy = torch.randn(3, 3, 12, 10, generator=_gen(7)).cuda()
    out = []
    for kw in ({}, {'resize_probs': None}):
        d = _degrader(**kw)
        xg = x.cuda().requires_grad_(True)
        y = d(xg, (12, 10))
        y.backward(dy)
        out.append((y.detach(), xg.grad))
        assert d.last_modes == [None, None] and d.resize_probs is None
    assert torch.equal(_bits(out[0][0]), _bits(out[1][0])) and torch.equal(_bits(out[0][1]), _bits(out[1][1]))
