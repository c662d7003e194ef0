"""GPU: the JPEG round trip (jpeg.py, csrc/jpeg.hip) against the float64 restatement of test_jpeg_cpu.py.

The rounding makes the operator discontinuous, so a value test needs inputs whose rounding decisions fp32 and float64 share:
  1. exact-decision inputs, built BACKWARDS from coefficients (k + delta) T with |delta| <= 0.3: every quotient is >= 0.2 away from
     a tie, the whole image is compared;
  2. natural inputs (the Pillow fixture's image, uniform noise beyond [-1, 1]) on ragged shapes with the clamp on: an MCU that holds
     a coefficient within 2.5e-4 of a tie in the restatement is left out -- more than 10 x the largest fp32-vs-float64 quotient
     difference measured (2.1e-5) -- and at most 15 % of the MCUs of a case may be.
Bounds: forward (64 + 64 + 16) 2^-23 max|p^| / 127.5 (the operation count of the two transforms and the colour arithmetic), backward
1e-5 max|dx|.  Shapes are the smallest at which each mechanism can go wrong (see SHAPES)."""
import sys

import numpy as np
import pytest
import torch

from gpu_helpers import pkg
from test_jpeg_cpu import COLOUR_INV, DCT, _unblocks, golden, jpeg64, mcu_of, tables_for

pytestmark = pytest.mark.gpu

SHAPES = [(1, 3, 8, 8),          # one block
          (2, 3, 16, 16),        # one 4:2:0 MCU; two samples with DIFFERENT qualities: sample b must use table b
          (1, 3, 3, 5),          # smaller than a block: the pad and its fold dominate
          (2, 3, 21, 37),        # ragged in both axes, odd W (no 16-byte access)
          (1, 1, 9, 7),          # grey: the luma table only
          (3, 3, 40, 52)]        # several workgroups
CASES = [(s, sub) for s in SHAPES for sub in (('444', '420') if s[1] == 3 else ('444',))]
_ids = ['%s_%s' % ('x'.join(map(str, s)), sub) for s, sub in CASES]
# the exact-decision test wants MCU multiples: the shapes above rounded up, and one that spans two tiles in both axes
EXACT_CASES = [((1, 3, 8, 8), '444'), ((2, 3, 16, 16), '444'), ((2, 3, 16, 16), '420'), ((1, 1, 16, 8), '444'), ((2, 3, 24, 40), '444'),
               ((3, 3, 32, 80), '444'), ((3, 3, 32, 80), '420')]
_exact_ids = ['%s_%s' % ('x'.join(map(str, s)), sub) for s, sub in EXACT_CASES]
QUALITIES = (50, 90, 10)         # of samples 0, 1, 2
AMBIGUOUS = 2.5e-4
CAP = 0.15


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _fwd_bound(y64):
    return (64 + 64 + 16) * 2.0 ** -23 * float(((y64 + 1) * 127.5).abs().max()) / 127.5


def _run(x32, tables, sub, grad, clamp, dy):
    """forward + backward on the device -> (y, dx) on the host"""
    J = pkg('jpeg')
    xg = x32.cuda().requires_grad_(True)
    y = J.jpeg_roundtrip(xg, tables.float().cuda(), sub, grad, clamp)
    y.backward(dy.cuda())
    return y.detach().cpu(), xg.grad.cpu()


# ---- 1. exact-decision inputs ---------------------------------------------------------------------------------------------------
def _exact_input(shape, sub, seed):
    """x (fp32) whose coefficients are (k + delta) T, k integer, |delta| <= 0.3, and its tables"""
    N, C, H, W = shape
    g = _gen(seed)
    tables = tables_for(QUALITIES[:N])
    s420 = mcu_of(C, sub) == 16
    planes = []
    for i in range(C):
        h, w = (H // 2, W // 2) if (s420 and i > 0) else (H, W)
        k = torch.randint(-2, 3, (N, h // 8, w // 8, 8, 8), generator=g).double()
        k[..., 0, 0] = torch.randint(-6, 7, (N, h // 8, w // 8), generator=g).double()
        delta = 0.6 * torch.rand(k.shape, generator=g, dtype=torch.float64) - 0.3
        c = (k + delta) * tables[:, min(i, 1), None, None]
        q = _unblocks(DCT.T @ c @ DCT)
        if s420 and i > 0:
            q = q.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
        planes.append(q if i > 0 else q + 128)
    p = torch.einsum('ij,njhw->nihw', COLOUR_INV, torch.stack(planes, dim=1)) if C == 3 else planes[0][:, None]
    return (p / 127.5 - 1).float(), tables


@pytest.mark.parametrize('shape,sub', EXACT_CASES, ids=_exact_ids)
def test_exact_decision_inputs(shape, sub):
    x32, tables = _exact_input(shape, sub, 100 + shape[2] + shape[3])
    dy = torch.randn(shape, generator=_gen(7))
    x64 = x32.double().requires_grad_(True)
    ref, us = jpeg64(x64, tables, sub, clamp=False, grad='ste', detail=True)
    away = min(float(((u - torch.round(u)).abs() - 0.5).abs().min().detach()) for u in us)
    assert away >= 0.19                                      # the construction: no quotient near a tie
    assert any(bool((torch.round(u)[..., 1:, 1:] != 0).any()) for u in us)
    bound = _fwd_bound(ref.detach())
    for grad in ('ste', 'cubic'):
        x64.grad = None
        jpeg64(x64, tables, sub, clamp=False, grad=grad).backward(dy.double())
        y, dx = _run(x32, tables, sub, grad, False, dy)
        err = float((y.double() - ref.detach()).abs().max())
        scale = float(x64.grad.abs().max())
        berr = float((dx.double() - x64.grad).abs().max())
        print('exact %s %s %s: forward max err %.3e (bound %.3e), backward max err / max |dx| %.3e' % (shape, sub, grad, err, bound, berr / scale))
        assert err <= bound
        assert scale > 0 and berr <= 1e-5 * scale
        if grad == 'ste' and sub == '444':                   # block multiples, no clamp: J^T is the identity
            assert float((dx - dy).abs().max()) <= 1e-5 * float(dy.abs().max())


# ---- 2. natural inputs, ragged shapes, clamp on ---------------------------------------------------------------------------------
def _natural_input(shape, kind, attempt):
    N, C, H, W = shape
    if kind == 'noise':
        return (2.4 * torch.rand(shape, generator=_gen(1000 + attempt)) - 1.2)
    img = torch.from_numpy(golden()['image'].astype(np.float32)) / 127.5 - 1            # [3, 40, 52]
    g = _gen(2000 + attempt)
    out = []
    for b in range(N):
        oy, ox = int(torch.randint(0, 40 - H + 1, (1,), generator=g)), int(torch.randint(0, 52 - W + 1, (1,), generator=g))
        out.append(img[:C, oy:oy + H, ox:ox + W] if C == 3 else img[(b + 1) % 3:(b + 1) % 3 + 1, oy:oy + H, ox:ox + W])
    return torch.stack(out)


def _compared_pixels(us, shape, sub):
    """-> (bool [N, 1, H, W]: the pixels of the MCUs without an ambiguous coefficient, the share of MCUs left out, whether a
    compared MCU holds a non-zero quantised AC coefficient)"""
    N, C, H, W = shape
    m = mcu_of(C, sub)
    amb, ac = None, None
    for u in us:
        r = torch.round(u)
        a = (((u - r).abs() - 0.5).abs() < AMBIGUOUS).flatten(3).any(-1).float()            # [N, by, bx]
        nz = r.clone()
        nz[..., 0, 0] = 0
        z = (nz != 0).flatten(3).any(-1).float()
        if m == 16 and a.shape[1] * 8 == -(-H // 16) * 16:                                  # luma blocks of 4:2:0: 2 x 2 per MCU
            a, z = torch.nn.functional.max_pool2d(a[:, None], 2)[:, 0], torch.nn.functional.max_pool2d(z[:, None], 2)[:, 0]
        amb = a if amb is None else torch.maximum(amb, a)
        ac = z if ac is None else torch.maximum(ac, z)
    keep = amb == 0
    pix = keep.repeat_interleave(m, dim=1).repeat_interleave(m, dim=2)[:, None, :H, :W]
    return pix, 1.0 - float(keep.float().mean()), bool((ac.bool() & keep).any())


@pytest.mark.parametrize('kind', ['image', 'noise'])
@pytest.mark.parametrize('shape,sub', CASES, ids=_ids)
def test_natural_inputs_outside_ambiguous_mcus(shape, sub, kind):
    N = shape[0]
    tables = tables_for(QUALITIES[:N])
    for attempt in range(32):              # the first input that compares enough MCUs, an AC coefficient and a clamped pixel
        x32 = _natural_input(shape, kind, attempt)
        with torch.no_grad():
            ref, us = jpeg64(x32.double(), tables, sub, clamp=True, detail=True)
        pix, left_out, has_ac = _compared_pixels(us, shape, sub)
        clamped = bool(((ref.abs() == 1) & pix).any())
        if left_out <= CAP and has_ac and clamped:
            break
    print('natural %s %s %s: attempt %d, %.1f %% of the MCUs left out' % (shape, sub, kind, attempt, 100 * left_out))
    assert left_out <= CAP and has_ac and clamped
    bound = _fwd_bound(ref)
    dy = torch.randn(shape, generator=_gen(9))
    for grad in ('ste', 'cubic'):
        y, dx = _run(x32, tables, sub, grad, True, dy)
        err = float(((y.double() - ref).abs() * pix).max())
        # the clamp's mask is the saved output by definition: the reference differentiates the unclamped operator under it
        mask = ((y > -1) & (y < 1)).double()
        x64 = x32.double().requires_grad_(True)
        jpeg64(x64, tables, sub, clamp=False, grad=grad).backward(dy.double() * mask)
        scale = float((x64.grad.abs() * pix).max())
        berr = float(((dx.double() - x64.grad).abs() * pix).max())
        print('   %s: forward max err %.3e (bound %.3e), backward max err / max |dx| %.3e' % (grad, err, bound, berr / scale))
        assert err <= bound
        assert scale > 0 and berr <= 1e-5 * scale
        assert bool(((mask == 0) & pix).any()) and bool(((mask == 1) & pix).any())


# ---- 3. adjoint identity ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,sub', CASES, ids=_ids)
def test_adjoint_identity(shape, sub):
    """<J v, w> = <v, J^T w> for 'ste' without the clamp.  The identity is one of LINEAR operators, and J^T under 'ste' is the
    transpose of J with the rounding taken out; tables of 2^-20 take it out of the forward too (rintf(c 2^20) 2^-20 is c to 2^-21,
    exactly c from |c| = 8 on), so both sides are the kernels' own.  Independent of the restatement: a wrong pad fold or chroma
    transpose fails here."""
    g = _gen(shape[2] * 100 + shape[3])
    v = 2 * torch.rand(shape, generator=g) - 1
    w = torch.randn(shape, generator=g)
    tables = torch.full((shape[0], 2, 8, 8), 2.0 ** -20)
    jv, jtw = _run(v, tables, sub, 'ste', False, w)
    lhs, rhs = float((jv.double() * w.double()).sum()), float((v.double() * jtw.double()).sum())
    scale = float((jv.double().abs() * w.double().abs()).sum())
    print('adjoint %s %s: |lhs - rhs| / sum |Jv| |w| %.3e' % (shape, sub, abs(lhs - rhs) / scale))
    assert abs(lhs - rhs) <= 1e-5 * scale


def test_the_three_forms_of_quality_agree():
    J = pkg('jpeg')
    x = (2 * torch.rand(2, 3, 21, 37, generator=_gen(11)) - 1).cuda()
    want = J.jpeg_roundtrip(x, tables_for((75, 75)).float().cuda())
    assert torch.equal(J.jpeg_roundtrip(x, 75), want) and torch.equal(J.jpeg_roundtrip(x, torch.tensor([75, 75])), want)
    assert not torch.equal(J.jpeg_roundtrip(x, torch.tensor([75, 20]).cuda()), want)
    for bad in (dict(quality=0), dict(quality=torch.tensor([75, 75, 75])), dict(quality=75.0), dict(subsampling='422'), dict(grad='soft')):
        with pytest.raises(ValueError):
            J.jpeg_roundtrip(x, **dict(dict(quality=75), **bad))


# ---- 4. draw ------------------------------------------------------------------------------------------------------------------------
def test_tables_launch_matches_the_host_and_leaves_the_step():
    D, J = pkg('degrade'), pkg('jpeg')
    d = D.Degrader(ksize=7, seed=77, rank=4, jpeg=(1, 100))
    d.load_state_dict(dict(seed=77, rank=4, step=(1 << 32) + 6))
    for t in ((1 << 32) + 6, (1 << 32) + 7):
        _, _, drawn = d.draw(300)
        tables = d.draw_jpeg_tables(300, drawn)
        assert int(drawn) == t and int(d.step) == t + 1                      # the tables launch read the step and left it
        q = d.last_quality.cpu().numpy()
        assert np.array_equal(q, J.expected_quality(77, t, 300, 1, 100, 4))
        want = np.stack([np.stack(J.quant_tables(int(v))) for v in q]).astype(np.float32)
        assert np.array_equal(tables.cpu().numpy(), want)
        assert q.min() < 10 and q.max() > 90


# ---- 5. determinism and capture -----------------------------------------------------------------------------------------------------
def _degrader(**kw):
    return pkg('degrade').Degrader(ksize=7, sigma=(0.5, 2.0), noise=(0., 0.05), seed=5, **kw)


@pytest.mark.parametrize('sub,grad', [('420', 'cubic'), ('444', 'ste')])
def test_two_calls_are_bit_equal(sub, grad):
    x = 1.2 * (2 * torch.rand(2, 3, 21, 37, generator=_gen(3)) - 1)
    dy = torch.randn(2, 3, 21, 37, generator=_gen(4))
    a, b = (_run(x, tables_for((30, 80)), sub, grad, True, dy) for _ in range(2))
    for u, v in zip(a, b):
        assert torch.equal(u.view(torch.int32), v.view(torch.int32))
    assert float(a[1].abs().max()) > 0


def test_captured_jpeg_degrader_advances_on_every_replay():
    G = pkg('graph')
    x = (2 * torch.rand(2, 3, 24, 40, generator=_gen(5)) - 1).cuda()
    d, twin = _degrader(jpeg=(30, 95)), _degrader(jpeg=(30, 95))
    step = G.GraphedStep(lambda: d(x, (12, 20)))
    t0 = int(d.step)
    twin.load_state_dict(dict(d.state_dict(), step=t0))
    got = [step().clone() for _ in range(3)]
    assert int(d.step) == t0 + 3
    want, qual = [], []
    for _ in range(3):
        want.append(twin(x, (12, 20)))
        qual.append(twin.last_quality.clone())
    for a, b in zip(got, want):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert not torch.equal(got[0], got[1]) and not torch.equal(got[1], got[2])
    assert not torch.equal(qual[0], qual[1]) and set(d.state_dict()) == {'seed', 'rank', 'step'}


def test_jpeg_none_is_todays_degrader():
    x = (2 * torch.rand(2, 3, 24, 40, generator=_gen(6)) - 1).cuda()
    a, b, c = _degrader(jpeg=None), _degrader(), _degrader(jpeg=(30, 95))
    ya, yb, yc = a(x, (12, 20)), b(x, (12, 20)), c(x, (12, 20))
    assert torch.equal(ya.view(torch.int32), yb.view(torch.int32)) and a.last_quality is None
    assert not torch.equal(yc, yb) and tuple(c.last_quality.shape) == (2,)
    # the JPEG switch appends to the same LR image and draws nothing else
    J = pkg('jpeg')
    assert torch.equal(c.last_kernels, b.last_kernels)
    assert torch.equal(yc, J.jpeg_roundtrip(yb, c.last_tables, '420'))


# ---- 6. install ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('grad', ['ste', 'cubic'])
def test_install_backpropagates_through_the_jpeg_degrader(grad):
    P = pkg()
    P.install()
    mod = sys.modules['utils']
    original = mod.lr_from_hr
    d = _degrader(jpeg=(30, 95), jpeg_grad=grad)
    fake = (2 * torch.rand(2, 3, 32, 32, generator=_gen(8)) - 1).cuda().requires_grad_(True)
    try:
        P.install(degradation=d)
        lr = sys.modules['utils'].lr_from_hr(fake, (16, 16), device='cuda')
        assert tuple(lr.shape) == (2, 3, 16, 16) and int(d.step) == 1
        lr.square().sum().backward()
    finally:
        mod.lr_from_hr = original
    assert bool(torch.isfinite(fake.grad).all()) and float(fake.grad.abs().max()) > 0
