"""GPU: the backward of the generator's last conv (3x3, 64 -> 3, + Tanh) in one launch -- toimage_bwd.hip behind
engine.toimage_backward -- against a float64 reference built with torch on the CPU (conv2d backward, tanh', PReLU slope gradient):
the data gradient g, the weight and bias gradients (through the slab sum and the un-packing the training step uses) and the slope
gradient of the last upscale stage.

Shapes (N, H, W[, workgroup cap]):
  (2, 8, 32)      one tile per image; every tile edge is an image edge
  (3, 24, 64, 5)  18 tiles, interior and edge ones, on 5 workgroup slots (SISR_PERSIST_MAX_WG): four workgroups walk 4 tiles, one 2
  (1, 13, 31)     not eligible: the three separate kernels, bit for bit what SISR_TOIMAGE_BWD=0 gives
each with and without the tanh' operand and with slopes 0.25, 0.0, 1.0.

grid inputs: every operand a small multiple of 1/8 (tanh output in {0, +-0.5}, pre with exact zeros and negatives), so that every
product and every partial sum of every output is exact in fp32 whatever the order: the four outputs must EQUAL the float64 reference.
The reference's sums of |terms| are checked to stay below 2^24 units of each output's grid.
random inputs U(-1, 1): per output err = max|out - ref64| / max|ref64|, measured for the fused launch and for the three separate
kernels on the same inputs; required: fused <= max(2 x separate, 2^-22) -- a different but equally long summation order, floor one
fp32 rounding."""
import pytest
import torch
import torch.nn.functional as F

from gpu_helpers import FakeConv, pkg

pytestmark = pytest.mark.gpu

SHAPES = [(2, 8, 32), (3, 24, 64, 5)]
SLOPES = [0.25, 0.0, 1.0]
KNOBS = ('SISR_TOIMAGE_BWD', 'SISR_THIN', 'SISR_PERSIST_MAX_WG', 'SISR_FUSE_SLABRED')


def _inputs(shape, kind, use_tanh, slope, seed=0):
    """CPU fp32 tensors: pre NHWC [N,H,W,64], dy / out NCHW [N,3,H,W] (out None without tanh'), W [3,64,3,3], bias [3], slope [1]"""
    n, h, w = shape[:3]
    gen = torch.Generator().manual_seed(1000 * seed + 7 * n + h + w)
    if kind == 'grid':
        def ints(size, lo, hi):
            return torch.randint(lo, hi + 1, size, generator=gen).float()
        pre = ints((n, h, w, 64), -2, 2) / 8
        dy = ints((n, 3, h, w), -1, 1) / 8
        out = ints((n, 3, h, w), -1, 1) / 2 if use_tanh else None
        wt = ints((3, 64, 3, 3), -1, 1) / 8
        assert bool((pre == 0).any()) and bool((pre < 0).any())
    else:
        def uni(size):
            return torch.rand(size, generator=gen) * 2 - 1
        pre, dy, wt = uni((n, h, w, 64)), uni((n, 3, h, w)), uni((3, 64, 3, 3))
        out = uni((n, 3, h, w)) if use_tanh else None
    return pre, dy, out, wt, torch.zeros(3), torch.tensor([slope])


def _reference(pre, dy, out, wt, slope):
    """float64 on the CPU -> (g NHWC, dW, db, dslope [1]) and, per output, the largest sum of |terms| (the grid bound)"""
    p = pre.double().permute(0, 3, 1, 2)
    s = slope.double().clone().requires_grad_(True)
    x = torch.where(p > 0, p, s * p)
    x.retain_grad()
    w64 = wt.double().clone().requires_grad_(True)
    b64 = torch.zeros(3, dtype=torch.float64, requires_grad=True)
    dyt = dy.double() * (1 - out.double() ** 2) if out is not None else dy.double()
    F.conv2d(x, w64, b64, padding=1).backward(dyt)
    g = x.grad.permute(0, 2, 3, 1).contiguous()
    # sums of |terms|: an upper bound of every partial sum in any order
    xa = x.detach().abs()
    abs_g = F.conv_transpose2d(dyt.abs(), wt.double().abs(), padding=1)
    abs_w = torch.autograd.grad(F.conv2d(xa, w64, padding=1), w64, dyt.abs())[0]
    abs_s = (abs_g * p.abs() * (p <= 0)).sum()
    mags = dict(g=float(abs_g.max()), dw=float(abs_w.max()), db=float(dyt.abs().sum((0, 2, 3)).max()), dslope=float(abs_s))
    return (g, w64.grad, b64.grad, s.grad.reshape(1)), mags


def _run(shape, pre, dy, out, wt, bias, slope, fused):
    """the end conv's backward as generator_engine.run_backward schedules it -> (g, dW, db, dslope) on the CPU, fused launches"""
    E, L = pkg('engine'), pkg('_lib')
    n, h, w = shape[:3]
    dev = 'cuda'
    wd, bd = wt.to(dev).requires_grad_(True), bias.to(dev).requires_grad_(True)
    sd = slope.to(dev).requires_grad_(True)
    ref = FakeConv(wd, bd, E.ConvGeom(64, 3, 3, 1, 1))
    preps, keep = E.prepare_weights([(ref, n, h, w)], True)
    book = E.BackwardBook({id(ref): preps[0]}, [ref], [], None, own_batch_slabs=True)
    pre_d, dy_d, out_d = pre.to(dev), dy.to(dev), None if out is None else out.to(dev)
    x_op = E.Operand.act(pre_d, sd)
    dy_op = E.Operand(dy_d, (n, h, w, 3), pro=L.PRO_TANH_BWD if out is not None else L.PRO_NONE, mode=L.X_NCHW, x2=out_d)
    before = E.KERNEL_COUNTS.get('toimage_bwd', 0)
    res = book.toimage_bwd(ref, x_op, dy_op) if fused else None
    if res is not None:
        g, dslope = res
    else:
        g = book.conv_bwd(ref, x_op, dy_op)
        dslope = E.prelu_slope_grad(g, pre_d)
    book.flush('end')
    torch.cuda.synchronize()
    launches = E.KERNEL_COUNTS.get('toimage_bwd', 0) - before
    return (g.cpu(), book.grads[id(wd)].cpu(), book.grads[id(bd)].cpu(), dslope.cpu()), launches


@pytest.fixture(autouse=True)
def _knobs(monkeypatch):
    for v in KNOBS:
        monkeypatch.delenv(v, raising=False)
    pkg('engine').set_precision('fp32')


def _cap(monkeypatch, shape):
    if len(shape) > 3:
        monkeypatch.setenv('SISR_PERSIST_MAX_WG', str(shape[3]))


NAMES = ('g', 'dw', 'db', 'dslope')
UNITS = dict(g=1 / 256, dw=1 / 1024, db=1 / 32, dslope=1 / 2048)        # grids: W dyt = 1/8 * 1/32; lrelu(pre, 1/4) dyt; dyt; g pre


@pytest.mark.parametrize('use_tanh', [True, False], ids=['tanh', 'plain'])
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_grid_inputs_equal_the_float64_reference(monkeypatch, shape, use_tanh):
    _cap(monkeypatch, shape)
    pre, dy, out, wt, bias, slope = _inputs(shape, 'grid', use_tanh, 0.25)
    ref, mags = _reference(pre, dy, out, wt, slope)
    for name in NAMES:
        units = mags[name] / UNITS[name]
        print('%s: sum of |terms| = %.0f grid units (2^24 = %d)' % (name, units, 2 ** 24))
        assert units < 2 ** 24, name
    got, launches = _run(shape, pre, dy, out, wt, bias, slope, fused=True)
    assert launches == 1
    for name, a, b in zip(NAMES, got, ref):
        assert a.dtype == torch.float32 and a.shape == b.shape, name
        assert torch.equal(a, b.float()), (name, float((a.double() - b).abs().max()))
    again, _ = _run(shape, pre, dy, out, wt, bias, slope, fused=True)
    assert all(torch.equal(a, b) for a, b in zip(got, again))


def _errors(got, ref):
    return [float((a.double() - b).abs().max() / b.abs().max()) for a, b in zip(got, ref)]


@pytest.mark.parametrize('slope', SLOPES)
@pytest.mark.parametrize('use_tanh', [True, False], ids=['tanh', 'plain'])
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_random_inputs_no_worse_than_the_three_kernels(monkeypatch, shape, use_tanh, slope):
    _cap(monkeypatch, shape)
    args = _inputs(shape, 'random', use_tanh, slope, seed=1)
    pre, dy, out, wt, bias, sl = args
    ref, _ = _reference(pre, dy, out, wt, sl)
    got, launches = _run(shape, *args, fused=True)
    assert launches == 1
    again, _ = _run(shape, *args, fused=True)
    for name, a, b in zip(NAMES, got, again):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), 'two runs differ: ' + name
    monkeypatch.setenv('SISR_TOIMAGE_BWD', '0')
    old, launches = _run(shape, *args, fused=True)              # (the library's switch: the same call falls back)
    assert launches == 0
    # the data gradient sums its 27 products in the generic kernel's order and the weight gradient in wgrad_toimage.hip's: same values
    for name, a, b in zip(NAMES[:3], got, old):
        assert torch.equal(a, b), 'differs from the separate kernels: ' + name
    e_new, e_old = _errors(got, ref), _errors(old, ref)
    for name, en, eo in zip(NAMES, e_new, e_old):
        print('%s: fused %.3e, three kernels %.3e' % (name, en, eo))
    for name, en, eo in zip(NAMES, e_new, e_old):
        assert en <= max(2 * eo, 2.0 ** -22), (name, en, eo)


@pytest.mark.parametrize('use_tanh', [True, False], ids=['tanh', 'plain'])
def test_an_odd_shape_keeps_the_three_kernels_bit_for_bit(monkeypatch, use_tanh):
    shape = (1, 13, 31)
    args = _inputs(shape, 'random', use_tanh, 0.25, seed=2)
    got, launches = _run(shape, *args, fused=True)
    assert launches == 0
    monkeypatch.setenv('SISR_TOIMAGE_BWD', '0')
    off, _ = _run(shape, *args, fused=True)
    plain, _ = _run(shape, *args, fused=False)
    for name, a, b, c in zip(NAMES, got, off, plain):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(a.view(torch.int32), c.view(torch.int32)), name
    ref, _ = _reference(*args[:4], args[5])
    assert max(_errors(got, ref)) < 1e-5


def _generator_grads(net, x, w_out):
    net.zero_grad(set_to_none=True)
    (net(x) * w_out).sum().backward()
    return [p.grad for p in net.parameters()]


def test_graph_replay_of_the_generator_backward(monkeypatch):
    """the smallest generator whose last conv runs at (3, 24, 64): forward + backward captured once (graph.GraphedStep), replayed
    twice: the gradients of the replays are identical and equal the eager launches'; the fused kernel is what ran"""
    E, G, mg = pkg('engine'), pkg('graph'), pkg('model_generator')
    monkeypatch.setenv('SISR_PERSIST_MAX_WG', '5')
    torch.manual_seed(3)
    net = mg.Generator(1, 64, 256, [2]).cuda().train()
    x = torch.rand(3, 3, 12, 32, device='cuda') * 2 - 1
    w_out = torch.rand(3, 3, 24, 64, device='cuda') - 0.5
    state = {k: v.clone() for k, v in net.state_dict().items()}
    before = E.KERNEL_COUNTS.get('toimage_bwd', 0)
    eager = [g.clone() for g in _generator_grads(net, x, w_out)]
    assert E.KERNEL_COUNTS.get('toimage_bwd', 0) == before + 1
    names = [k for k, _ in net.named_parameters()]

    net.load_state_dict(state)
    step = G.GraphedStep(lambda: _generator_grads(net, x, w_out), warmup=1)
    replays = []
    for _ in range(2):
        net.load_state_dict(state)              # (spectral-norm vectors and running statistics advance with every forward)
        replays.append([g.clone() for g in step()])
    torch.cuda.synchronize()
    for k, a, b, c in zip(names, replays[0], replays[1], eager):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), 'replays differ: ' + k
        assert torch.equal(a.view(torch.int32), c.view(torch.int32)), 'replay differs from eager: ' + k
