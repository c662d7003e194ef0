"""GPU: losses.frequency_loss / fft_l1_loss / focal_frequency_loss (csrc/freq_loss.hip), forward and backward, against the
definition evaluated in float64 on the CPU from the same fp32 inputs (freq_cases.py: torch.fft.rfft2 / fft2 + autograd), for the
upstream gradient 1 + 0.5 n.

Cases (freq_cases.CASES): each the smallest shape at which one thing can go wrong -- DC alone, all-real bins, Nyquist row / column,
odd / even mixes (Wh, Hermitian weights), ragged 8-line blocks, the crop / luma view, the training sizes with the longest sums.
All three kinds run on every case; the L1 GRADIENT is compared only where the sign margin condition holds
(freq_cases.L1_GRAD_CASES, asserted by test_freq_loss_cpu.py): elsewhere some |Re D| or |Im D| is too close to 0 for its sign to be
safe in fp32, one flipped sign moves the whole gradient by about 2 / sqrt(count), and 'charbonnier' and 'focal' check the same
backward kernels.

Bounds, the project's own (test_gpu_image_loss.py): |loss - ref| <= 2e-5 |ref| (relative: these losses span 1e-6 .. 17) and
max|grad - ref| <= 1e-4 max|ref| for da and db.  The definition evaluated in fp32 on the CPU is within 2.8e-7 and 9.7e-6 of the
float64 one (test_freq_loss_cpu.py prints it per case)."""
import pytest
import torch
import torch.nn.functional as F

from freq_cases import CASES, KINDS, L1_GRAD_CASES, _reference, upstream
from gpu_helpers import SENT, Buf, pkg, run2
from image_cases import _images

pytestmark = pytest.mark.gpu

FWD_TOL = 2e-5
GRAD_TOL = 1e-4


def _fused(shape, crop, luma, kind, seed=0, want_a=True, want_b=True, **kw):
    """forward + backward on the device -> (loss [N], da or None, db or None)"""
    Lo = pkg('losses')
    a, b = (t.cuda() for t in _images(shape, seed))
    a.requires_grad_(want_a)
    b.requires_grad_(want_b)
    loss = Lo.frequency_loss(a, b, kind=kind, crop_border=crop, luma=luma, reduction='none', **kw)
    (loss * upstream(shape[0], torch.float32).cuda()).sum().backward()
    return loss.detach(), a.grad, b.grad


def _grad_err(got, want):
    return float((got.double().cpu() - want).abs().max() / want.abs().max())


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('shape,crop,luma', CASES)
def test_loss_and_gradients_match_the_float64_definition(shape, crop, luma, kind):
    want, want_da, want_db, _ = _reference(shape, crop, luma, kind)
    loss, da, db = _fused(shape, crop, luma, kind)
    assert loss.shape == (shape[0],) and loss.dtype == torch.float32 and loss.is_cuda
    assert da.shape == shape and db.shape == shape and da.dtype == torch.float32
    e_fwd = float(((loss.double().cpu() - want).abs() / want.abs()).max())
    e_a, e_b = _grad_err(da, want_da), _grad_err(db, want_db)
    grads = kind != 'l1' or (shape, crop, luma) in L1_GRAD_CASES
    print('frequency_loss %s crop %d luma %d %s: loss rel err %.3g, da err %.3g, db err %.3g of max|ref|%s'
          % (shape, crop, luma, kind, e_fwd, e_a, e_b, '' if grads else ' (gradient not compared: sign margin)'))
    assert e_fwd <= FWD_TOL
    assert bool(torch.isfinite(da).all()) and bool(torch.isfinite(db).all())
    if grads:
        assert e_a <= GRAD_TOL and e_b <= GRAD_TOL


@pytest.mark.parametrize('alpha', [0.5, 2.0, 4.0])
def test_focal_alpha(alpha):
    shape, crop, luma = (2, 3, 21, 36), 2, False
    want, want_da, want_db, _ = _reference(shape, crop, luma, 'focal', alpha)
    loss, da, db = _fused(shape, crop, luma, 'focal', alpha=alpha)
    e_fwd = float(((loss.double().cpu() - want).abs() / want.abs()).max())
    e_a, e_b = _grad_err(da, want_da), _grad_err(db, want_db)
    print('frequency_loss focal alpha %g: loss rel err %.3g, da err %.3g, db err %.3g of max|ref|' % (alpha, e_fwd, e_a, e_b))
    assert e_fwd <= FWD_TOL and e_a <= GRAD_TOL and e_b <= GRAD_TOL


def test_charbonnier_eps():
    shape, crop, luma = (2, 3, 21, 36), 0, False
    want, want_da, want_db, _ = _reference(shape, crop, luma, 'charbonnier', 1.0, 0.5)
    loss, da, db = _fused(shape, crop, luma, 'charbonnier', eps=0.5)
    assert float(((loss.double().cpu() - want).abs() / want.abs()).max()) <= FWD_TOL
    assert _grad_err(da, want_da) <= GRAD_TOL and _grad_err(db, want_db) <= GRAD_TOL


def test_structurally_real_bins_give_the_same_l1_gradient_in_every_pixel():
    """(1, 1, 2, 2): all four bins are real, Im D is exactly 0 and contributes sign(0) = 0: the gradient of every pixel is
    +-(1 / 8) (sum of four signs), a multiple of 1 / 8 exactly"""
    _, da, db = _fused((1, 1, 2, 2), 0, False, 'l1')
    assert torch.equal(da * 8, (da * 8).round()) and torch.equal(db, -da)
    _, da1, _ = _fused((1, 1, 1, 1), 0, False, 'l1')
    assert float(da1.abs().max()) == 0.5              # mean over {Re, Im} of one bin: |Re D| / 2


@pytest.mark.parametrize('shape,crop,luma', [((2, 3, 21, 36), 2, True), ((1, 3, 45, 70), 1, False), ((1, 3, 96, 96), 4, True),
                                             ((2, 3, 40, 24), 3, False)])
def test_cropped_border_gets_exact_zeros_from_a_dirty_allocator(shape, crop, luma):
    """the gradients are torch.empty: blocks that held NaNs are handed back to the backward, which must write every element"""
    Lo = pkg('losses')
    for kind in ('charbonnier', 'focal'):
        a, b = (t.cuda().requires_grad_() for t in _images(shape))
        loss = Lo.frequency_loss(a, b, kind=kind, crop_border=crop, luma=luma)
        dirty = [torch.full(shape, float('nan'), device='cuda') for _ in range(2)]
        del dirty                                    # two free blocks of the gradients' size, full of NaNs
        loss.backward()
        for grad in (a.grad, b.grad):
            assert bool(torch.isfinite(grad).all())
            inner = torch.zeros(shape, dtype=torch.bool, device='cuda')
            inner[:, :, crop:shape[2] - crop, crop:shape[3] - crop] = True
            assert bool((grad[~inner] == 0).all())
            assert bool((grad[inner] != 0).any())


@pytest.mark.parametrize('kind', KINDS)
def test_db_is_minus_da_bit_for_bit_and_only_the_requested_gradient_is_produced(kind):
    shape, crop = (2, 3, 17, 33), 1
    loss2, da2, db2 = _fused(shape, crop, False, kind)
    assert torch.equal(db2, -da2)
    loss1, da1, db1 = _fused(shape, crop, False, kind, want_b=False)
    assert db1 is None and torch.equal(da1, da2) and torch.equal(loss1, loss2)
    loss0, da0, db0 = _fused(shape, crop, False, kind, want_a=False)
    assert da0 is None and torch.equal(db0, db2) and torch.equal(loss0, loss2)
    Lo = pkg('losses')
    a, b = (t.cuda() for t in _images(shape))
    assert not Lo.frequency_loss(a, b, kind=kind).requires_grad
    with torch.no_grad():
        assert torch.equal(Lo.frequency_loss(a.requires_grad_(), b, kind=kind, crop_border=crop, reduction='none'), loss2)


def test_luma_gradients_are_the_luma_gradient_times_the_coefficients():
    _, da, db = _fused((2, 3, 21, 36), 2, True, 'charbonnier')
    assert torch.equal(db, -da)
    g = da.double().cpu()
    nz = g[:, 0] != 0
    assert int(nz.sum()) >= 2 * 17 * 32 - 4
    assert float((g[:, 1][nz] / g[:, 0][nz] - 0.587 / 0.299).abs().max()) <= 1e-6
    assert float((g[:, 2][nz] / g[:, 0][nz] - 0.114 / 0.299).abs().max()) <= 1e-6


def test_focal_equal_images_give_exact_zero_and_no_nan_beside_a_different_image():
    """image 0: a == b in every plane; image 1 differs.  Also one equal PLANE inside a differing image"""
    Lo = pkg('losses')
    shape = (2, 3, 21, 36)
    a0, b0 = (t.cuda() for t in _images(shape))
    b0 = b0.clone()
    b0[0] = a0[0]
    b0[1, 1] = a0[1, 1]
    a, b = a0.clone().requires_grad_(), b0.clone().requires_grad_()
    loss = Lo.focal_frequency_loss(a, b, reduction='none')
    (loss * upstream(2, torch.float32).cuda()).sum().backward()
    loss = loss.detach()
    assert float(loss[0]) == 0.0 and float(loss[1]) > 0.0
    for grad in (a.grad, b.grad):
        assert bool(torch.isfinite(grad).all())
        assert bool((grad[0] == 0).all()) and bool((grad[1, 1] == 0).all())
        assert bool((grad[1, 0] != 0).any()) and bool((grad[1, 2] != 0).any())
    a64, b64 = (t.double().cpu().requires_grad_() for t in (a0, b0))
    from freq_cases import defn
    want = defn(a64, b64, 'focal')[0]
    want_da, = torch.autograd.grad((want * upstream(2)).sum(), a64)
    assert abs(float(loss[1]) - float(want[1])) <= FWD_TOL * float(want[1])
    assert _grad_err(a.grad, want_da) <= GRAD_TOL


def test_two_calls_are_bit_equal():
    for kind, view in (('l1', (0, False)), ('charbonnier', (4, True)), ('focal', (2, False))):
        first, second = _fused((1, 3, 96, 192), *view, kind), _fused((1, 3, 96, 192), *view, kind)
        assert all(torch.equal(x, y) for x, y in zip(first, second))


def test_non_contiguous_inputs_equal_their_contiguous_copies():
    Lo = pkg('losses')
    shape = (2, 3, 45, 70)
    a0, b0 = (t.cuda() for t in _images(shape))
    want = _fused(shape, 2, False, 'focal')
    g = upstream(2, torch.float32).cuda()
    cl = [t.contiguous(memory_format=torch.channels_last) for t in (a0, b0)]
    sl = [F.pad(t, (2, 3, 1, 1), value=0.5)[:, :, 1:-1, 2:-3] for t in (a0, b0)]
    for a, b in (cl, sl):
        assert not a.is_contiguous() and torch.equal(a, a0)
        a, b = a.detach().requires_grad_(), b.detach().requires_grad_()
        loss = Lo.frequency_loss(a, b, kind='focal', crop_border=2, reduction='none')
        (loss * g).sum().backward()
        assert torch.equal(loss.detach(), want[0])
        assert a.grad.shape == shape and torch.equal(a.grad, want[1]) and torch.equal(b.grad, want[2])


def test_reductions_and_wrappers():
    Lo = pkg('losses')
    a, b = (t.cuda() for t in _images((2, 3, 45, 70)))
    for kind in KINDS:
        none = Lo.frequency_loss(a, b, kind=kind, crop_border=1, reduction='none')
        mean = Lo.frequency_loss(a, b, kind=kind, crop_border=1)
        assert none.shape == (2,) and mean.shape == () and mean.dtype == torch.float32 and mean.is_cuda
        assert torch.equal(mean, none.mean())
    assert torch.equal(Lo.fft_l1_loss(a, b, crop_border=2, luma=True), Lo.frequency_loss(a, b, kind='l1', crop_border=2, luma=True))
    assert torch.equal(Lo.fft_l1_loss(a, b, reduction='none'), Lo.frequency_loss(a, b, reduction='none'))
    assert torch.equal(Lo.focal_frequency_loss(a, b, alpha=2.0, crop_border=1),
                       Lo.frequency_loss(a, b, kind='focal', alpha=2.0, crop_border=1))
    assert torch.equal(Lo.focal_frequency_loss(a, b, luma=True, reduction='none'),
                       Lo.frequency_loss(a, b, kind='focal', luma=True, reduction='none'))


def test_side_257_raises_value_error_before_any_launch():
    Lo = pkg('losses')
    for shape in ((1, 1, 8, 257), (1, 3, 257, 8)):
        t = torch.zeros(shape, device='cuda')
        with pytest.raises(ValueError):
            Lo.frequency_loss(t, t.clone())
    t = torch.zeros(1, 1, 258, 8, device='cuda')
    with pytest.raises(ValueError):
        Lo.frequency_loss(t, t.clone())
    assert float(Lo.frequency_loss(t, t.clone(), crop_border=1)) == 0.0          # 256 x 6 left: legal


def test_longest_side_and_a_prime_side():
    """256 (the limit) x 13 and 127 (a prime: no FFT-friendly factor) x 256, one plane: values and gradients"""
    from freq_cases import evaluate
    for shape in ((1, 1, 256, 13), (1, 1, 127, 256)):
        for kind in ('charbonnier', 'focal'):
            want, want_da, want_db, _ = evaluate(shape, 0, False, kind, torch.float64)
            loss, da, db = _fused(shape, 0, False, kind)
            e_fwd = float(((loss.double().cpu() - want).abs() / want.abs()).max())
            e_a, e_b = _grad_err(da, want_da), _grad_err(db, want_db)
            print('frequency_loss %s %s: loss rel err %.3g, da err %.3g, db err %.3g of max|ref|' % (shape, kind, e_fwd, e_a, e_b))
            assert e_fwd <= FWD_TOL and e_a <= GRAD_TOL and e_b <= GRAD_TOL


@pytest.mark.parametrize('kind', [0, 2])
@pytest.mark.parametrize('shape,crop,luma', [((2, 3, 21, 36), 2, 1), ((1, 3, 45, 70), 0, 0), ((1, 1, 17, 256), 0, 0)])
def test_c_abi_writes_stay_inside_their_buffers(shape, crop, luma, kind):
    """every output of the five launches between sentinel guards, sized by the workspace query; two runs, identical bits"""
    L = pkg('_lib')
    lib = L.lib()
    n = shape[0]
    a, b = (t.cuda() for t in _images(shape))
    g = upstream(n, torch.float32).cuda()
    ws = [lib.sisr_freq_loss_ws_floats(*shape, crop, luma, which) for which in range(4)]
    assert min(ws) > 0
    work, spec, pmax, loss, work2 = Buf(ws[0]), Buf(ws[1]), Buf(ws[2]), Buf(n), Buf(ws[3])
    da, db = Buf(a.numel()), Buf(a.numel())
    stream = torch.cuda.current_stream().cuda_stream
    run2(lambda: lib.sisr_freq_loss_fwd(a.data_ptr(), b.data_ptr(), *shape, crop, luma, kind, 1e-3, 1.0, work.ptr(), spec.ptr(),
                                        pmax.ptr(), loss.ptr(), stream), [work, spec, pmax, loss])
    assert bool((spec.body != SENT).all()) and bool((loss.body != SENT).all())
    run2(lambda: lib.sisr_freq_loss_bwd(spec.ptr(), pmax.ptr(), g.data_ptr(), *shape, crop, luma, kind, 1e-3, 1.0, work2.ptr(),
                                        da.ptr(), db.ptr(), stream), [work2, da, db])
    assert bool((da.body != SENT).all()) and torch.equal(db.body, -da.body)


def test_launch_sequence_is_capturable_and_replays_on_new_contents():
    """no host synchronisation on the path: GraphedStep captures forward + backward (a GraphCaptureError fails the test) and a
    replay after new contents were copied into the static inputs equals an eager call on those contents"""
    Lo, G = pkg('losses'), pkg('graph')
    shape = (2, 3, 45, 70)
    a0, b0 = (t.cuda() for t in _images(shape))
    a1, b1 = (t.cuda() for t in _images(shape, seed=1))
    g = upstream(2, torch.float32).cuda()
    for kind, luma in (('charbonnier', True), ('focal', False)):
        def fwd_bwd(a, b):
            a, b = a.detach().requires_grad_(), b.detach().requires_grad_()
            loss = Lo.frequency_loss(a, b, kind=kind, crop_border=2, luma=luma, reduction='none')
            return (loss,) + torch.autograd.grad((loss * g).sum(), (a, b))
        sa, sb = a0.clone(), b0.clone()
        step = G.GraphedStep(lambda: fwd_bwd(sa, sb))
        out, eager0 = step(), fwd_bwd(a0, b0)
        assert all(torch.equal(x, y) for x, y in zip(out, eager0))
        sa.copy_(a1)
        sb.copy_(b1)
        out, eager1 = step(), fwd_bwd(a1, b1)
        assert not torch.equal(eager1[0], eager0[0])
        assert all(torch.equal(x, y) for x, y in zip(out, eager1))
