"""GPU: losses.feature_mse / bce_loss / BCELoss and the three train.py loss functions (csrc/losses.hip) against the definitions
evaluated in float64 on the CPU from the same fp32 inputs and the fp32-rounded scalars (weight, upstream gradient, target).

Feature MSE.  Inputs are structured (a smooth pattern plus noise whose strength grows along the index, never constant), so a dropped
tail or a double-counted block moves the result far beyond the bound.  The kernel's tile is 4 x 256 16-byte loads = 4096 elements,
the grid is capped at 2048 workgroups: n = 1, 3, 4, 5 live in the peeled head / tail alone, 255 and 1025 in one ragged tile,
20011 = 4 full tiles + a ragged one (also run with SISR_PERSIST_MAX_WG=3: two sweeps of a 3-workgroup grid), 2^21 + 5 = 512 full
tiles + a ragged one.  Each size also runs on a contiguous view with storage offset 1 (4-byte, not 16-byte aligned: a 3-element
head is peeled in the forward; the backward, whose fresh gradient tensors sit at another offset, takes the one-element path), and
the backward's peeled-head path is driven through the C ABI with gradient buffers at the inputs' offset.
Bounds: forward relative 1e-5 (all terms are non-negative, so the error is at most (longest fp32 addition chain + a few) x 2^-24;
the chain is <= 2 sweeps + 2 + 6 + 3 additions here); gradient elementwise relative 1e-6 against c (b - a), c = 2 weight g / n
(three fp32 roundings, 1.8e-7).

BCE.  Reference: torch.nn.BCELoss on the CPU in float64 with the target rounded to fp32 first.  Forward relative 1e-5 with absolute
floor 1e-7, gradient elementwise relative 1e-5, mean(p) relative 1e-6."""
import functools
import importlib
import sys

import numpy as np
import pytest
import torch

from gpu_helpers import PKG, pkg
from helpers import grads_close, rel_err

pytestmark = pytest.mark.gpu

MSE_SIZES = [1, 3, 4, 5, 255, 1025, 20011, 2 ** 21 + 5]
BCE_SIZES = [1, 16, 64, 65, 257, 1000]
BCE_SPECIALS = [0.0, 1.0, 2.0 ** -24, 1.0 - 2.0 ** -24, 1e-30]
MSE_FWD_TOL, MSE_GRAD_TOL = 1e-5, 1e-6
BCE_FWD_TOL, BCE_FWD_FLOOR, BCE_GRAD_TOL, MEAN_TOL = 1e-5, 1e-7, 1e-5, 1e-6


def f32(v):
    return float(np.float32(v))


@functools.lru_cache(maxsize=None)
def _vectors(n, seed=0):
    """(a, b) fp32 CPU vectors; never modified"""
    x = torch.linspace(0, 1, n, dtype=torch.float64)
    i = torch.arange(n, dtype=torch.float64)
    base = 0.8 * torch.sin(0.37 * i + 5.0 * x + seed) * (0.3 + 0.7 * x) + 0.05
    noise = torch.randn(n, dtype=torch.float64, generator=torch.Generator().manual_seed(4321 + seed))
    return base.float(), (base + noise * (0.02 + 0.25 * x)).float()


def _place(t, offset):
    """device copy of t: a fresh tensor, or a contiguous view with storage offset 1 (4-byte but not 16-byte aligned)"""
    if not offset:
        return t.cuda()
    big = torch.zeros(t.numel() + 8, device='cuda')
    view = big[1:t.numel() + 1]
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view.detach()


def _mse_reference(a, b, weight, g=1.0):
    """-> (loss, db) in float64; da = -db"""
    a, b = a.double(), b.double()
    w, g = f32(weight), f32(g)
    return w * float(((a - b) ** 2).mean()), (2.0 * w * g / a.numel()) * (b - a)


def _rel(got, want):
    return abs(float(got) - want) / abs(want)


def _elem_ok(got, want, tol):
    """elementwise |got - want| <= tol |want| -> (ok, worst relative error over the non-zero reference elements)"""
    got, want = got.detach().double().cpu().reshape(-1), want.reshape(-1)
    err = (got - want).abs()
    nz = want != 0
    worst = float((err[nz] / want[nz].abs()).max()) if bool(nz.any()) else 0.0
    return bool((err <= tol * want.abs()).all()), worst


@pytest.mark.parametrize('offset', [0, 1])
@pytest.mark.parametrize('n', MSE_SIZES)
def test_feature_mse_matches_the_float64_definition(n, offset):
    Lo = pkg('losses')
    a0, b0 = _vectors(n)
    for weight, up in ((1.0, 1.0), (10.0, 3.0)):
        a, b = _place(a0, offset).requires_grad_(), _place(b0, offset).requires_grad_()
        loss = Lo.feature_mse(a, b, weight)
        assert loss.shape == () and loss.dtype == torch.float32 and loss.device == a.device
        (loss if up == 1.0 else up * loss).backward()
        want, want_db = _mse_reference(a0, b0, weight, up)
        ok_b, worst_b = _elem_ok(b.grad, want_db, MSE_GRAD_TOL)
        ok_a, worst_a = _elem_ok(a.grad, -want_db, MSE_GRAD_TOL)
        print('feature_mse n %d offset %d weight %g upstream %g: loss rel err %.3g, grad rel err %.3g / %.3g'
              % (n, offset, weight, up, _rel(loss, want), worst_a, worst_b))
        assert _rel(loss, want) <= MSE_FWD_TOL
        assert ok_a and ok_b, (worst_a, worst_b)
        assert torch.equal(a.grad, -b.grad)
        assert a.grad.shape == a.shape and b.grad.shape == b.shape


def test_feature_mse_sweeps_a_small_grid_several_times(monkeypatch):
    Lo = pkg('losses')
    monkeypatch.setenv('SISR_PERSIST_MAX_WG', '3')
    n = 20011
    a0, b0 = _vectors(n)
    a, b = a0.cuda().requires_grad_(), b0.cuda().requires_grad_()
    loss = Lo.feature_mse(a, b)
    loss.backward()
    torch.cuda.synchronize()
    want, want_db = _mse_reference(a0, b0, 1.0)
    ok_b, worst_b = _elem_ok(b.grad, want_db, MSE_GRAD_TOL)
    print('feature_mse n %d on 3 workgroups: loss rel err %.3g, grad rel err %.3g' % (n, _rel(loss, want), worst_b))
    assert _rel(loss, want) <= MSE_FWD_TOL
    assert ok_b and torch.equal(a.grad, -b.grad)


@pytest.mark.parametrize('n', [3, 5, 1025, 20011])
def test_mse_backward_peels_the_head_when_the_gradients_share_the_inputs_offset(n):
    """the 16-byte path of the backward with a 3-element head: every pointer at storage offset 1, through the C ABI"""
    L, E = pkg('_lib'), pkg('engine')
    a0, b0 = _vectors(n)
    a, b = _place(a0, 1), _place(b0, 1)
    guard = 7.0
    da_big, db_big = (torch.full((n + 8,), guard, device='cuda') for _ in range(2))
    g = torch.tensor(3.0, device='cuda')
    L.check(L.lib().sisr_mse_bwd(a.data_ptr(), b.data_ptr(), g.data_ptr(), n, 10.0, da_big[1:].data_ptr(), db_big[1:].data_ptr(),
                                 E._stream()), 'sisr_mse_bwd')
    _, want_db = _mse_reference(a0, b0, 10.0, 3.0)
    ok_b, worst = _elem_ok(db_big[1:n + 1], want_db, MSE_GRAD_TOL)
    assert ok_b, worst
    assert torch.equal(da_big[1:n + 1], -db_big[1:n + 1])
    for big in (da_big, db_big):                               # nothing outside [1, n + 1) was written
        assert float(big[0]) == guard and bool((big[n + 1:] == guard).all())


def test_feature_mse_computes_only_the_gradients_asked_for():
    Lo = pkg('losses')
    n = 1025
    a0, b0 = _vectors(n)
    _, want_db = _mse_reference(a0, b0, 1.0)
    a, b = a0.cuda(), b0.cuda().requires_grad_()
    Lo.feature_mse(a, b).backward()
    assert a.grad is None and _elem_ok(b.grad, want_db, MSE_GRAD_TOL)[0]
    a, b = a0.cuda().requires_grad_(), b0.cuda()
    Lo.feature_mse(a, b).backward()
    assert b.grad is None and _elem_ok(a.grad, -want_db, MSE_GRAD_TOL)[0]
    assert not Lo.feature_mse(a0.cuda(), b0.cuda()).requires_grad


def test_feature_mse_non_contiguous_inputs_equal_their_contiguous_copies():
    Lo = pkg('losses')
    a0, b0 = _vectors(37 * 53)
    at, bt = a0.cuda().view(37, 53).t(), b0.cuda().view(37, 53).t()
    assert not at.is_contiguous()
    a, b = at.detach().requires_grad_(), bt.detach().requires_grad_()
    ac, bc = at.contiguous().requires_grad_(), bt.contiguous().requires_grad_()
    assert not a.is_contiguous() and ac.is_contiguous()
    loss, loss_c = Lo.feature_mse(a, b, 10.0), Lo.feature_mse(ac, bc, 10.0)
    loss.backward()
    loss_c.backward()
    assert torch.equal(loss, loss_c)
    assert a.grad.shape == a.shape and torch.equal(a.grad, ac.grad) and torch.equal(b.grad, bc.grad)
    want, _ = _mse_reference(at.cpu(), bt.cpu(), 10.0)
    assert _rel(loss, want) <= MSE_FWD_TOL


# ---- BCE ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _probs(n, seed=0):
    """fp32 CPU vector of n probabilities: random in (0, 1), the exact edge values in front where they fit; never modified"""
    p = torch.rand(n, dtype=torch.float64, generator=torch.Generator().manual_seed(99 + seed)).float().clamp(1e-6, 1 - 1e-6)
    if n >= 16 and seed == 0:
        p[:len(BCE_SPECIALS)] = torch.tensor(BCE_SPECIALS, dtype=torch.float64).float()
    return p


@functools.lru_cache(maxsize=None)
def _targets(n):
    return torch.rand(n, dtype=torch.float64, generator=torch.Generator().manual_seed(7)).float()


def _bce_reference(p, target, weight, g=1.0):
    """torch.nn.BCELoss on the CPU in float64 -> (loss, dp, mean p)"""
    p64 = p.double().requires_grad_()
    t64 = target.double() if isinstance(target, torch.Tensor) else torch.full_like(p64, f32(target))
    loss = torch.nn.BCELoss()(p64, t64.detach())
    loss.backward()
    return f32(weight) * float(loss), f32(weight) * f32(g) * p64.grad, float(p.double().mean())


@pytest.mark.parametrize('target', [1.0, 0.9, 0.0, 'tensor'])
@pytest.mark.parametrize('n', BCE_SIZES)
def test_bce_matches_torch_in_float64(n, target):
    Lo = pkg('losses')
    p0 = _probs(n)
    t0 = _targets(n) if target == 'tensor' else target
    for weight, up in ((1.0, 1.0), (5e-2, 3.0)):
        p = p0.cuda().requires_grad_()
        t = t0.cuda() if target == 'tensor' else t0
        loss, mean_p = Lo.bce_loss(p, t, weight, return_mean=True)
        for v in (loss, mean_p):
            assert v.shape == () and v.dtype == torch.float32 and v.device == p.device
        assert not mean_p.requires_grad
        (loss if up == 1.0 else up * loss).backward()
        want, want_dp, want_mean = _bce_reference(p0, t0, weight, up)
        ok, worst = _elem_ok(p.grad, want_dp, BCE_GRAD_TOL)
        print('bce n %d target %s weight %g upstream %g: loss %.6g err %.3g, grad rel err %.3g, mean err %.3g'
              % (n, target, weight, up, want, abs(float(loss) - want), worst, _rel(mean_p, want_mean)))
        assert abs(float(loss) - want) <= max(BCE_FWD_TOL * abs(want), BCE_FWD_FLOOR)
        assert ok, worst
        assert _rel(mean_p, want_mean) <= MEAN_TOL
        assert torch.equal(Lo.bce_loss(p.detach(), t, weight), loss.detach())
    if target == 'tensor':
        assert torch.equal(Lo.BCELoss()(p0.cuda(), t0.cuda()), Lo.bce_loss(p0.cuda(), t0.cuda()))


def test_bce_forward_clamps_the_logarithm_at_minus_100():
    Lo = pkg('losses')
    for weight in (1.0, 10.0):
        assert float(Lo.bce_loss(torch.zeros(1, device='cuda'), 1.0, weight)) == 100.0 * weight
        assert float(Lo.bce_loss(torch.ones(1, device='cuda'), 0.0, weight)) == 100.0 * weight
    assert float(Lo.bce_loss(torch.zeros(1, device='cuda'), 0.0)) == 0.0


def test_bce_gradient_uses_torch_s_epsilon():
    Lo = pkg('losses')
    n = 6
    p = torch.full((n,), 0.5, device='cuda')
    p[0] = 0.0
    p.requires_grad_()
    Lo.bce_loss(p, 1.0).backward()
    want = -1.0 / 1e-12 / n                                     # -1.6667e11
    assert abs(float(p.grad[0]) - want) <= BCE_GRAD_TOL * abs(want)
    assert abs(float(p.grad[1]) - (0.5 - 1.0) / 0.25 / n) <= BCE_GRAD_TOL * (0.5 / 0.25 / n)


def test_bce_nan_in_gives_nan_out_and_raises_nothing():
    Lo = pkg('losses')
    p0 = _probs(16).clone()
    p0[3] = float('nan')
    p = p0.cuda().requires_grad_()
    loss, mean_p = Lo.bce_loss(p, 0.9, return_mean=True)
    loss.backward()
    torch.cuda.synchronize()
    assert bool(torch.isnan(loss)) and bool(torch.isnan(mean_p))
    assert bool(torch.isnan(p.grad[3])) and bool(torch.isfinite(p.grad[5:]).all())
    # the device is still usable
    assert float(Lo.bce_loss(torch.full((4,), 0.5, device='cuda'), 1.0)) == pytest.approx(0.6931472, rel=1e-6)


# ---- determinism and capture ----------------------------------------------------------------------------------------------------
def _both_losses(a, b, p):
    """forward + backward of both losses -> six tensors"""
    Lo = pkg('losses')
    a, b, p = (t.detach().requires_grad_() for t in (a, b, p))
    mse = Lo.feature_mse(a, b, 2.0)
    bce, mean_p = Lo.bce_loss(p, 0.9, 5e-2, return_mean=True)
    ga, gb, gp = torch.autograd.grad(mse + bce, (a, b, p))
    return mse, bce, mean_p, ga, gb, gp


def test_two_calls_are_bit_equal():
    a, b = (t.cuda() for t in _vectors(20011))
    p = _probs(257).cuda()
    first, second = _both_losses(a, b, p), _both_losses(a, b, p)
    assert all(torch.equal(x, y) for x, y in zip(first, second))


def test_launch_sequence_is_capturable_and_replays_on_new_contents():
    """no host synchronisation on the path: GraphedStep captures forward + backward of both losses (a GraphCaptureError fails the
    test) and a replay after new contents were copied into the static inputs equals an eager call on those contents"""
    G = pkg('graph')
    a0, b0 = (t.cuda() for t in _vectors(20011))
    a1, b1 = (t.cuda() for t in _vectors(20011, seed=1))
    p0, p1 = _probs(257).cuda(), _probs(257, seed=1).cuda()
    sa, sb, sp = a0.clone(), b0.clone(), p0.clone()
    step = G.GraphedStep(lambda: _both_losses(sa, sb, sp))
    out = step()
    eager = _both_losses(a0, b0, p0)
    assert all(torch.equal(x, y) for x, y in zip(out, eager))
    sa.copy_(a1)
    sb.copy_(b1)
    sp.copy_(p1)
    out = step()
    eager1 = _both_losses(a1, b1, p1)
    assert not torch.equal(eager1[0], eager[0]) and not torch.equal(eager1[1], eager[1])
    assert all(torch.equal(x, y) for x, y in zip(out, eager1))


# ---- one training iteration -----------------------------------------------------------------------------------------------------
def test_one_training_iteration_with_the_fused_losses_matches_oracle(monkeypatch):
    """the sequence of test_gpu_train_step.test_one_training_iteration_matches_oracle (same nets, seed and HR batch, same bounds)
    with the loss glue replaced by losses.adversarial_loss_d / adversarial_loss_g / content_loss_g; the D statistics they return
    are the means of the oracle's three D outputs"""
    from test_gpu_train_step import FEATS, STRIDES, TOL, _oracle_iteration
    from oracle import models as om
    mg, md, mce, ut, Lo = pkg('model_generator'), pkg('model_discriminator'), pkg('model_content_extractor'), pkg('utils'), pkg('losses')
    d_means, forward = [], om.discriminator_forward

    def recording_forward(*args, **kw):
        out = forward(*args, **kw)
        d_means.append(float(out[0].detach().double().mean()))
        return out
    monkeypatch.setattr(om, 'discriminator_forward', recording_forward)
    torch.manual_seed(0)
    net_g = mg.Generator(2, 16, 64, [2], use_sn=True)
    net_d = md.Discriminator((3, 32, 32), FEATS, STRIDES)
    mask = 0b00011
    ext = mce.MaskedVGG(mask, width_div=4, pretrained=False)
    g_state = {k: v.detach().clone() for k, v in net_g.state_dict().items()}
    d_state = {k: v.detach().clone() for k, v in net_d.state_dict().items()}
    v_state = {k: v.detach().clone() for k, v in ext.state_dict().items()}
    hr = torch.rand(8, 3, 32, 32, generator=torch.Generator().manual_seed(3)) * 2 - 1
    ref = _oracle_iteration(g_state, d_state, v_state, hr, mask, (16, 16))
    assert len(d_means) == 3                                   # D(real), D(fake.detach()), D(fake)

    dev = torch.device('cuda')
    net_g, net_d, ext = net_g.to(dev), net_d.to(dev), ext.to(dev)
    img_hr = hr.to(dev)
    img_lr = ut.lr_from_hr(img_hr, (16, 16), device=dev)
    fake = net_g(img_lr)
    net_d.zero_grad()
    d_g_z1, d_x, err_d = Lo.adversarial_loss_d(net_d, img_hr, fake.detach(), [], weight=1.0)
    err_d.backward()
    d_grads = {k: p.grad.detach().cpu().clone() for k, p in net_d.named_parameters()}
    net_g.zero_grad()
    d_g_z2, err_adv = Lo.adversarial_loss_g(net_d, fake, weight=5e-2)
    err_cont = Lo.content_loss_g(ext, img_hr, fake)
    (err_adv + err_cont).backward()
    g_grads = {k: p.grad.detach().cpu() for k, p in net_g.named_parameters()}

    for t in (d_g_z1, d_x, d_g_z2, err_d, err_adv, err_cont):
        assert isinstance(t, torch.Tensor) and t.is_cuda and t.dim() == 0
    assert abs(float(err_d) - float(ref[0])) < TOL * max(1.0, abs(float(ref[0])))
    assert abs(float(err_adv) - float(ref[1])) < TOL * max(1.0, abs(float(ref[1])))
    assert abs(float(err_cont) - float(ref[2])) < TOL * max(1e-3, abs(float(ref[2])))
    assert grads_close(d_grads, ref[3], TOL) == []
    assert grads_close(g_grads, ref[4], 2 * TOL) == []
    sd = net_d.state_dict()
    for k, v in ref[5].items():
        assert rel_err(sd[k].cpu(), v) < TOL, k
    for got, want in zip((d_x, d_g_z1, d_g_z2), d_means):
        assert abs(float(got) - want) < TOL * abs(want), (float(got), want)


def test_install_with_fused_losses_points_torch_bce_at_the_fused_module():
    names = ('model_generator', 'model_generator_progressive', 'model_discriminator', 'model_content_extractor', 'utils')
    saved = {k: sys.modules.get(k) for k in names}
    original = torch.nn.BCELoss
    try:
        importlib.import_module(PKG).install(fused_losses=True)
        assert torch.nn.BCELoss is pkg('losses').BCELoss
        crit = torch.nn.BCELoss()                               # config.py:107
        p = _probs(16).cuda()
        assert torch.equal(crit(p, torch.full((16,), 0.9, device='cuda')), pkg('losses').bce_loss(p, 0.9))
    finally:
        torch.nn.BCELoss = original
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    assert torch.nn.BCELoss is original
