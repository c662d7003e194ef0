"""GPU: whole-image super-resolution in tiles (upscale.py, csrc/tiles.hip).

Kernel values without a network: SR tiles cut by torch slicing out of a known image must stitch back to it -- bit for bit without
feathering, within the fp32 rounding of the weighted sum (2e-5 absolute: values in [-1, 1], at most 32 weighted terms) with it --
and the fp32 gather must equal torch slicing plus flips / transposition bit for bit.  End to end: the tiled result is compared with
the WHOLE-IMAGE forward of the same net in eval mode (never with itself) under the project's 1e-3 parity bound between two fp32
evaluations of a forward (helpers.rel_err; 3e-2 in the bf16 build, the bound of test_gpu_bf16_mode.py).  Measured on an MI355X:
0 in all three builds -- these kernels sum every output pixel in an order that does not depend on where the pixel lies in its
tensor, so the two evaluations agree bit for bit -- against 0.27 to 0.37 with a halo of 4 instead of 12."""
import numpy as np
import pytest
import torch

from conftest import F32_TENSOR_BUILDS
from gpu_helpers import pkg
from helpers import rel_err

pytestmark = pytest.mark.gpu
SUM_TOL = 2e-5


def _image(shape, seed, lo=-1.0, hi=1.0):
    return (torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) * (hi - lo) + lo).cuda()


def _normalise(img_u8):
    """ToTensor + Normalize(.5, .5) of a [H, W, C] uint8 image -> [C, H, W] fp32 on the device, in numpy: two correctly rounded
    fp32 divisions, the gather's expressions (torch's division by a scalar on the device multiplies by a reciprocal)"""
    x = img_u8.cpu().numpy().astype(np.float32) / np.float32(255.0)
    x = (x - np.float32(0.5)) / np.float32(0.5)
    return torch.from_numpy(np.ascontiguousarray(x.transpose(2, 0, 1))).cuda()


def _ops(t, e):
    """hflip, vflip, transposition of the last two dimensions, in that order, as bits 0, 1, 2 of e say"""
    if e & 1:
        t = t.flip(-1)
    if e & 2:
        t = t.flip(-2)
    if e & 4:
        t = t.transpose(-1, -2)
    return t


def _inverse_ops(t, e):
    if e & 4:
        t = t.transpose(-1, -2)
    if e & 2:
        t = t.flip(-2)
    if e & 1:
        t = t.flip(-1)
    return t


def _cut(img, plan, s, E=1):
    """the SR tiles of every member, by torch slicing: [E n, C, s th, s tw]"""
    rows = []
    for e in range(E):
        for _, y0, x0, _ in plan.table.tolist():
            rows.append(_ops(img[:, s * y0:s * (y0 + plan.th), s * x0:s * (x0 + plan.tw)], e))
    return torch.stack(rows).contiguous()


def _stitch(dp, tiles, s, halo, f, E=1, u8=False, mean=0.5, std=0.5):
    p, C_ = dp.plan, tiles.shape[1]
    dst = (torch.zeros((s * p.H, s * p.W, C_), dtype=torch.uint8, device='cuda') if u8
           else torch.full((C_, s * p.H, s * p.W), -7.0, device='cuda'))
    status = pkg('_lib').lib().sisr_tile_stitch(tiles.data_ptr(), dp.table.data_ptr(), dp.ay.data_ptr(), dp.by.data_ptr(), p.ny,
                                                dp.ax.data_ptr(), dp.bx.data_ptr(), p.nx, C_, p.H, p.W, p.th, p.tw, s, halo, float(f),
                                                E, mean, std, dst.data_ptr(), int(u8), torch.cuda.current_stream().cuda_stream)
    assert status == 0, status
    return dst


def _weighted_constants(U, plan, s, f, c):
    """fp64 numpy restatement: sum over tiles of w * c at every output pixel -> [s H, s W]"""
    wy, wx = U.axis_weights(plan.by, s, f, plan.H), U.axis_weights(plan.bx, s, f, plan.W)
    return np.einsum('iy,jx,ij->yx', wy, wx, np.asarray(c, dtype=np.float64).reshape(plan.ny, plan.nx))


# ---- stitch values without a network -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('s', [2, 4])
@pytest.mark.parametrize('hw', [(45, 61), (11, 61)])
def test_stitch_without_feather_copies_the_owning_tile(hw, s):
    U = pkg('upscale')
    plan = U.TilePlan(hw[0], hw[1], 16, 3)
    assert (plan.th, plan.tw) == (min(16, hw[0]), 16) and plan.n == (4 if hw[0] == 45 else 1) * 6
    dp = U._DevicePlan(plan, 1, 'cuda')
    img = _image((3, s * hw[0], s * hw[1]), 1)
    out = _stitch(dp, _cut(img, plan, s), s, 3, 0)
    assert torch.equal(out.view(torch.int32), img.view(torch.int32))
    # a constant per tile shows WHICH tile every pixel was copied from: the owner
    c = torch.linspace(-0.5, 0.5, plan.n)
    out = _stitch(dp, _cut(img * 0.5, plan, s) + c.cuda()[:, None, None, None], s, 3, 0)
    want = (img * 0.5).double().cpu() + torch.from_numpy(_weighted_constants(U, plan, s, 0, c.numpy()))
    assert torch.equal(out.cpu(), want.float())            # fp32 x + c, the same single rounding on both sides


@pytest.mark.parametrize('f', [1, 3])
@pytest.mark.parametrize('s', [2, 4])
@pytest.mark.parametrize('hw', [(45, 61), (11, 61)])
def test_stitch_feathered_equals_the_fp64_restatement(hw, s, f):
    U = pkg('upscale')
    plan = U.TilePlan(hw[0], hw[1], 16, 3)
    dp = U._DevicePlan(plan, 1, 'cuda')
    img = _image((3, s * hw[0], s * hw[1]), 2, -0.5, 0.5)
    c = torch.rand(plan.n, generator=torch.Generator().manual_seed(3)) - 0.5
    tiles = _cut(img, plan, s) + c.cuda()[:, None, None, None]
    out = _stitch(dp, tiles, s, 3, f)
    shift = _weighted_constants(U, plan, s, f, c.numpy())
    assert np.ptp(shift) > 0.3                              # the constants are visible in the result
    want = img.double().cpu() + torch.from_numpy(shift)
    err = float((out.double().cpu() - want).abs().max())
    print('feathered stitch %s x%d f=%d: max abs err %.3e' % (hw, s, f, err))
    assert err <= SUM_TOL


@pytest.mark.parametrize('f', [0, 3])
@pytest.mark.parametrize('s', [2, 4])
def test_stitch_ensemble_undoes_every_members_operations(s, f):
    U = pkg('upscale')
    plan = U.TilePlan(45, 61, 16, 3)
    dp = U._DevicePlan(plan, 8, 'cuda')
    assert dp.table[:, 3].cpu().tolist() == [e for e in range(8) for _ in range(plan.n)]
    img = _image((3, s * 45, s * 61), 4)
    tiles = _cut(img, plan, s, E=8)
    out = _stitch(dp, tiles, s, 3, f, E=8)
    err = float((out.double() - img.double()).abs().max())
    print('ensemble stitch x%d f=%d: max abs err %.3e' % (s, f, err))
    assert err <= SUM_TOL
    # a constant per MEMBER: the result moves by their mean (every member is weighted 1 / 8, none twice)
    k = torch.tensor([0.5, -0.25, 0.125, 0.0, -0.5, 0.25, -0.125, 0.0625]).cuda()
    out = _stitch(dp, tiles * 0.5 + k.repeat_interleave(plan.n)[:, None, None, None], s, 3, f, E=8)
    err = float((out.double() - (img.double() * 0.5 + float(k.double().mean()))).abs().max())
    assert err <= SUM_TOL


def _quantise64(v64, mean, std):
    """fp64 restatement of the uint8 output: (q, distance of the value before floor from the nearest integer)"""
    p = (v64 * std + mean) * 255.0 + 0.5
    q = np.clip(np.floor(p), 0, 255)
    q[np.isnan(p)] = 0
    return q.astype(np.int64), np.abs(p - np.round(p))


@pytest.mark.parametrize('f,mean,std', [(0, 0.5, 0.5), (3, 0.5, 0.5), (1, 0.4, 0.3)])
def test_stitch_uint8_output(f, mean, std):
    U = pkg('upscale')
    s, plan = 2, U.TilePlan(45, 61, 16, 3)
    dp = U._DevicePlan(plan, 1, 'cuda')
    img = _image((3, s * 45, s * 61), 5, -1.3, 1.3)         # beyond +-1: both ends saturate
    img[0, 10, 20:24] = float('nan')
    img[2, 57, 0] = float('nan')
    img[1, 0, 0], img[1, 0, 1] = 1e30, -1e30
    out = _stitch(dp, _cut(img, plan, s), s, 3, f, u8=True, mean=mean, std=std)
    assert out.shape == (s * 45, s * 61, 3) and out.dtype == torch.uint8
    want, dist = _quantise64(img.double().cpu().numpy().transpose(1, 2, 0), mean, std)
    got = out.cpu().numpy().astype(np.int64)
    assert (got[10, 20:24, 0] == 0).all() and got[57, 0, 2] == 0                          # NaN -> 0
    assert got[0, 0, 1] == 255 and got[0, 1, 1] == 0                                      # values beyond the range saturate
    if (mean, std) == (0.5, 0.5):                           # ... as does the tenth of this image beyond +-1 at either end
        assert (got == 0).mean() > 0.05 and (got == 255).mean() > 0.05
    off = got != want
    near = dist < 1e-3
    print('uint8 stitch f=%d: %d of %d differ, %.3f %% of the values within 1e-3 of an integer'
          % (f, int(off.sum()), off.size, 100.0 * near.mean()))
    assert near.mean() < 0.01
    assert not (off & ~near).any() and (np.abs(got - want)[off] <= 1).all()


# ---- fp32 gather ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('th,tw,ops', [(16, 16, range(8)), (40, 40, range(8)), (16, 24, range(4)), (40, 35, range(4)),
                                       (45, 61, range(4))])
def test_tile_gather_f32_equals_torch_slicing(th, tw, ops):
    H, W = 45, 61
    src = _image((3, H, W), 6)
    g = torch.Generator().manual_seed(7)
    rows = []
    for e in ops:
        for y0, x0 in ((0, 0), (H - th, W - tw), (int(torch.randint(0, H - th + 1, (1,), generator=g)),
                                                  int(torch.randint(0, W - tw + 1, (1,), generator=g)))):
            rows.append((0, y0, x0, e))
    if th != tw:
        rows.append((0, 0, 0, 5))                           # bit 2 is ignored while th != tw
    rows += [(3, -4, W, 0), (0, H, -1, 3)]                  # out-of-range rows are clamped into the image
    table = torch.tensor(rows, dtype=torch.int32).cuda()
    n = len(rows)
    dst = torch.full((n, 3, th, tw), -7.0, device='cuda')
    status = pkg('_lib').lib().sisr_tile_gather_f32(src.data_ptr(), 3, H, W, table.data_ptr(), n, th, tw, dst.data_ptr(),
                                                    torch.cuda.current_stream().cuda_stream)
    assert status == 0
    for k, (_, y0, x0, e) in enumerate(rows):
        y0, x0 = min(max(y0, 0), H - th), min(max(x0, 0), W - tw)
        want = _ops(src[:, y0:y0 + th, x0:x0 + tw], e if th == tw else e & 3)
        assert torch.equal(dst[k].view(torch.int32), want.contiguous().view(torch.int32)), (k, rows[k])


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def _net(scales, use_sn, seed=11, blocks=2):
    mg, layers = pkg('model_generator'), pkg('layers')
    torch.manual_seed(seed)
    net = mg.Generator(blocks, 16, 64, scales, use_sn=use_sn).cuda().train()
    # non-trivial running statistics that fit the weights (made-up ones drive tanh into saturation, where every comparison passes):
    # 24 training-mode forwards over a noise batch take them 92 % of the way to its batch statistics (momentum 0.1)
    cal = _image((2, 3, 24, 24), seed + 1)
    with torch.no_grad():
        for _ in range(24):
            net(cal)
    bns = [m for m in net.modules() if isinstance(m, layers.BatchNorm2d)]
    assert bns and all(int(m.num_batches_tracked) == 24 for m in bns) and any(float((m.running_var - 1).abs().max()) > 0.05 for m in bns)
    return net


def _whole(net, image, check=True):
    modes = [(m, m.training) for m in net.modules()]
    net.eval()
    with torch.no_grad():
        out = net(image[None])[0]
    for m, was in modes:
        m.training = was
    if check:                                               # an image with content, not a saturated tanh
        assert float(out.abs().max()) < 0.999 and float(out.std()) > 0.02
    return out


@pytest.mark.parametrize('f32_build', F32_TENSOR_BUILDS, indirect=True)
@pytest.mark.parametrize('use_sn', [False, True])
@pytest.mark.parametrize('scales', [[2], [2, 2]])
def test_tiled_upscale_equals_the_whole_image_forward(scales, use_sn, f32_build):
    U = pkg('upscale')
    net = _net(scales, use_sn)
    up = U.Upscaler(net, tile=32, batch=4)
    assert up.halo == 12 and up.scale == 2 ** len(scales) and up.plan(45, 61).n == 15
    image = _image((3, 45, 61), 12)
    out = up(image)
    ref = _whole(net, image)
    assert out.shape == ref.shape == (3, up.scale * 45, up.scale * 61)
    err = rel_err(out.cpu(), ref.cpu())
    print('tiled vs whole x%d sn=%s %s: rel_err %.3e' % (up.scale, use_sn, f32_build, err))
    assert err <= 1e-3


def test_tiled_upscale_in_the_bf16_build():
    U, E = pkg('upscale'), pkg('engine')
    E.set_precision('bf16')
    try:
        net = _net([2], True)
        image = _image((3, 45, 61), 12)
        out = U.Upscaler(net, tile=32, batch=4)(image)
        err = rel_err(out.cpu(), _whole(net, image).cpu())
    finally:
        E.set_precision('fp32')
    print('tiled vs whole, bf16 build: rel_err %.3e' % err)
    assert err < 3e-2


@pytest.mark.parametrize('hw,n', [((20, 27), 1), ((32, 32), 1), ((32, 61), 5), ((33, 32), 2)])
def test_images_smaller_than_or_exactly_one_tile(hw, n):
    U = pkg('upscale')
    net = _net([2], True)
    up = U.Upscaler(net, tile=32, batch=4)
    assert up.plan(*hw).n == n                              # core 32 - 2 * 12 = 8: ceil((61 - 24) / 8) = 5, ceil((33 - 24) / 8) = 2
    image = _image((3,) + hw, 13)
    assert rel_err(up(image).cpu(), _whole(net, image).cpu()) <= 1e-3


def test_feathered_and_small_halo_results_stay_close_to_the_exact_one():
    """A feathered seam blends pixels up to `feather` beyond the ownership boundary, so it averages EQUAL values -- and the result
    stays the whole-image forward -- where halo >= receptive halo + feather.  A smaller halo is an approximation -- on this noise
    image a visible one, which also shows that the comparison with the whole-image forward can fail -- and stays an image (finite,
    inside tanh's range), feathered or not"""
    U = pkg('upscale')
    net = _net([2], False)
    image = _image((3, 45, 61), 12)
    ref = _whole(net, image)
    assert rel_err(U.Upscaler(net, tile=48, halo=12 + 5, feather=5, batch=16)(image).cpu(), ref.cpu()) <= 1e-3
    for feather in (0, 4):
        out = U.Upscaler(net, tile=32, halo=4, feather=feather, batch=16)(image)
        err = rel_err(out.cpu(), ref.cpu())
        print('halo 4 of 12, feather %d: rel_err %.3e' % (feather, err))
        assert err > 1e-3 and bool(torch.isfinite(out).all()) and float(out.abs().max()) <= 1.0


def test_self_ensemble_equals_the_mean_of_eight_whole_image_forwards():
    U = pkg('upscale')
    net = _net([2], True)
    image = _image((3, 45, 61), 14)
    out = U.Upscaler(net, tile=32, batch=16, ensemble=8)(image)
    ref = torch.zeros_like(out)
    for e in range(8):
        ref += _inverse_ops(_whole(net, _ops(image, e).contiguous()), e)
    ref *= 0.125
    err = rel_err(out.cpu(), ref.cpu())
    print('ensemble tiled vs whole: rel_err %.3e' % err)
    assert err <= 1e-3
    assert rel_err(out.cpu(), _whole(net, image).cpu()) > 1e-3        # ... and it is not the plain forward
    with pytest.raises(ValueError, match='would work'):
        U.Upscaler(net, tile=32, ensemble=8)(_image((3, 20, 61), 14))


def test_uint8_in_and_out():
    U = pkg('upscale')
    net = _net([2, 2], False)
    up = U.Upscaler(net, tile=32, batch=4)
    img = torch.randint(0, 256, (45, 61, 3), generator=torch.Generator().manual_seed(15), dtype=torch.uint8).cuda()
    sr = up.to_float(img)
    assert sr.shape == (3, 180, 244) and sr.dtype == torch.float32
    # the same tiles, hence the same bits
    norm = _normalise(img)
    assert torch.equal(sr, up(norm))
    out = up(img)
    assert out.shape == (180, 244, 3) and out.dtype == torch.uint8
    want = torch.floor((sr * 0.5 + 0.5) * 255.0 + 0.5).clamp(0, 255).to(torch.uint8).permute(1, 2, 0)
    assert torch.equal(out, want)
    assert rel_err(sr.cpu(), _whole(net, norm).cpu()) <= 1e-3
    assert out.float().std() > 5                            # an image, not a constant


def test_evaluate_image_equals_the_manual_pipeline():
    U, M, ut = pkg('upscale'), pkg('metrics'), pkg('utils')
    net = _net([2], True)
    up = U.Upscaler(net, tile=32, batch=4)
    hr_u8 = torch.randint(0, 256, (90, 122, 3), generator=torch.Generator().manual_seed(16), dtype=torch.uint8).cuda()
    got = U.evaluate_image(up, hr_u8)
    hr = _normalise(hr_u8)[None]
    sr = up(ut.lr_from_hr(hr, (45, 61))[0])
    p, s = M.psnr_ssim(sr[None], hr, crop_border=2)
    assert sorted(got) == ['psnr', 'ssim'] and torch.equal(got['psnr'], p) and torch.equal(got['ssim'], s)
    assert bool(torch.isfinite(p).all())
    with pytest.raises(ValueError):
        U.evaluate_image(up, hr_u8[:89])


# ---- state -------------------------------------------------------------------------------------------------------------------------
def _snapshot(net):
    return {k: v.clone() for k, v in net.state_dict().items()}, [m.training for m in net.modules()]


def _assert_untouched(net, snap):
    state, modes = snap
    after = net.state_dict()
    assert list(after.keys()) == list(state.keys())
    changed = [k for k in state if not torch.equal(state[k], after[k])]
    assert not changed, changed
    assert [m.training for m in net.modules()] == modes


def test_the_generator_is_left_as_it_was_also_when_the_forward_raises():
    U = pkg('upscale')
    net = _net([2], True)
    net.block_list[1].eval()                                # a mixed pattern of training flags
    snap = _snapshot(net)
    assert any('running_mean' in k for k in snap[0]) and any(k.endswith('_u') for k in snap[0]) and True in snap[1] and False in snap[1]
    up = U.Upscaler(net, tile=32, batch=4)
    image = _image((3, 45, 61), 12)
    up(image)
    _assert_untouched(net, snap)
    calls, forward = [], net.forward

    def failing(x):
        calls.append(net.training)
        if len(calls) == 2:
            raise RuntimeError('boom')
        return forward(x)
    net.forward = failing
    try:
        with pytest.raises(RuntimeError, match='boom'):
            up(image)
    finally:
        del net.forward
    assert calls == [False, False]                          # eval mode inside, the second slice raised
    _assert_untouched(net, snap)


def test_ema_weights_are_applied_and_the_live_ones_come_back():
    U, EMA = pkg('upscale'), pkg('ema')
    net = _net([2], True)
    ema = EMA.WeightEMA(net, decay=0.5)
    with torch.no_grad():
        for p in net.parameters():                          # the live weights move away from the average
            p.add_(torch.randn(p.shape, generator=torch.Generator().manual_seed(p.numel())).cuda() * 0.05)
    snap = _snapshot(net)
    image = _image((3, 45, 61), 12)
    out = U.Upscaler(net, tile=32, batch=4, ema=ema)(image)
    _assert_untouched(net, snap)
    live = _whole(net, image, check=False)
    with ema.applied():
        averaged = _whole(net, image)
    _assert_untouched(net, snap)
    assert rel_err(out.cpu(), averaged.cpu()) <= 1e-3 and rel_err(out.cpu(), live.cpu()) > 1e-2
    with pytest.raises(ValueError):
        U.Upscaler(_net([2], True), ema=ema)

    def failing(x):
        raise RuntimeError('boom')
    net.forward = failing
    try:
        with pytest.raises(RuntimeError, match='boom'):
            U.Upscaler(net, tile=32, batch=4, ema=ema)(image)
    finally:
        del net.forward
    _assert_untouched(net, snap)


# ---- determinism -------------------------------------------------------------------------------------------------------------------
def test_two_calls_are_bit_equal():
    U = pkg('upscale')
    net = _net([2], True)
    image = _image((3, 45, 61), 12)
    up = U.Upscaler(net, tile=32, batch=4, feather=3)
    a, b = up(image), up(image)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    up8 = U.Upscaler(net, tile=32, batch=16, ensemble=8, feather=2)
    assert torch.equal(up8(image).view(torch.int32), up8(image).view(torch.int32))


def test_stitch_launch_is_capturable_and_replays_on_new_tile_contents():
    U, G = pkg('upscale'), pkg('graph')
    s, plan = 2, U.TilePlan(45, 61, 16, 3)
    dp = U._DevicePlan(plan, 8, 'cuda')
    up = U.Upscaler(_net([2], False), tile=16, halo=3, feather=2, ensemble=8)
    t0 = _cut(_image((3, s * 45, s * 61), 20), plan, s, E=8)
    t1 = _cut(_image((3, s * 45, s * 61), 21), plan, s, E=8) + 0.25
    static = t0.clone()
    dst = torch.empty((3, s * 45, s * 61), device='cuda')
    step = G.GraphedStep(lambda: up.stitch(static, dp, dst))
    eager0 = _stitch(dp, t0, s, 3, 2, E=8)
    assert torch.equal(step().view(torch.int32), eager0.view(torch.int32))
    static.copy_(t1)
    eager1 = _stitch(dp, t1, s, 3, 2, E=8)
    assert not torch.equal(eager1, eager0)
    assert torch.equal(step().view(torch.int32), eager1.view(torch.int32))


# ---- command-line tool ---------------------------------------------------------------------------------------------------------------
def test_command_line_tool_writes_the_upscaled_image(tmp_path, capsys):
    """tools/upscale_image.py, in process: checkpoint in the reference's layout + PNG in -> the PNG that Upscaler gives for the same
    weights; --ema takes the averaged weights stored beside them"""
    import importlib
    import os
    import sys
    from PIL import Image
    U = pkg('upscale')
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    try:
        T = importlib.import_module('upscale_image')
    finally:
        sys.path.pop(0)
    net, other = _net([2], True), _net([2], True, seed=31)
    state = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    state_ema = {k: v.detach().cpu().clone() for k, v in other.state_dict().items()}
    ckpt, src, dst = (str(tmp_path / n) for n in ('ckpt.pth', 'in.png', 'out.png'))
    torch.save({'epoch': 3, 'net_g': state, 'net_g_ema': state_ema, 'net_d': {}, 'opti_g': {}, 'opti_d': {}, 'dis_list': []}, ckpt)
    img = torch.randint(0, 256, (45, 61, 3), generator=torch.Generator().manual_seed(32), dtype=torch.uint8)
    Image.fromarray(img.numpy()).save(src)
    for flags, ref_net in (([], net), (['--ema'], other)):
        T.main([ckpt, src, dst, '--tile', '32', '--batch', '4'] + flags)
        assert '45 -> ' in capsys.readouterr().out
        got = torch.from_numpy(np.asarray(Image.open(dst)).copy())
        want = U.Upscaler(ref_net, tile=32, batch=4)(img.cuda()).cpu()
        assert got.shape == (90, 122, 3) and torch.equal(got, want)
    assert not torch.equal(U.Upscaler(net, tile=32)(img.cuda()), U.Upscaler(other, tile=32)(img.cuda()))
    with pytest.raises(SystemExit):
        T.main([ckpt, src, dst, '--ema', '--tile', '0'])
