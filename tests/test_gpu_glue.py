"""GPU: value tests of the glue kernels between the convolutions -- layout changes, 2x2 max-pooling, the element-wise passes,
the generic fully connected kernels and the BatchNorm constants -- one entry point at a time through the C ABI, against torch on
the CPU in float64 (fp32 where the operation is a pure selection or movement and must be bit-exact).

What every case does:
  * the outputs live inside larger device buffers whose borders (and, for strided destinations, the gaps between the slots) hold a
    sentinel that must still be there afterwards -- an out-of-range store shows up as a changed guard, never as a fault;
  * every launch runs twice from the same pre-fill and must give the same bits;
  * bounds come from the number formats, not from what the kernels return (u = 2^-24, the fp32 unit round-off):
      - selection / movement / ONE fp32 operation per element: bit-exact against torch fp32 (IEEE), bf16 outputs against
        ref32.to(bfloat16) (the store is the hardware's round-to-nearest-even), bf16 inputs are built by rounding on the host so both
        sides read the same values;
      - an affine or a product the compiler may fuse:  |got - ref64| <= 2^-23 * sum|terms|  (+ 2^-8 * |ref64| for a bf16 store);
      - fp32 reductions:  |got - ref64| <= 2 * D * 2^-24 * sum|terms|, D = the longest chain of fp32 additions a result passes
        through, counted from the kernel beside each case;
      - bn_finalize sums in double: 4 * 2^-24 relative against a float64 Chan merge of the SAME fp32-rounded per-tile partials.
Grid caps (blocks x 256 threads, one work item per thread and trip) are restated beside the case that runs past them."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gpu_helpers import BF16, F32, GUARD, SENT, Buf, _bits, assert_within, pkg, run2

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
DT = {0: F32, 1: BF16}
BADARG, UNSUPPORTED = -1, -3


@pytest.fixture(scope='module')
def lib():
    return pkg('_lib').lib()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def dev(t, dtype=F32):
    return t.to(dtype).contiguous().cuda()


def lrelu64(v, slope):
    return torch.where(v > 0, v, v * float(np.float32(slope)))


# ---- transposes ---------------------------------------------------------------------------------------------------------------
# 32 x 32 (pixel x channel) tiles: HW = 35, 64, 66, 32 and C = 3, 40, 130, 64 give partial tiles on either side, several
# channel tiles and an exact fit
T_SHAPES = [(2, 5, 7, 3), (1, 8, 8, 40), (3, 6, 11, 130), (2, 4, 8, 64)]


def _rows(N, CHW, wide):
    """(row stride, offset of the slot in its row): the packed form, and a wider row with the slot in the middle -- a tap written
    into its place in the concatenated feature row"""
    return (CHW + 24, 8) if wide else (CHW, 0)


@pytest.mark.parametrize('x_bf16', [0, 1])
@pytest.mark.parametrize('shape', T_SHAPES)
def test_nhwc_to_nchw(lib, shape, x_bf16):
    N, H, W, C = shape
    HW, CHW = H * W, C * H * W
    x = torch.randn(N, H, W, C, generator=_gen(1)).to(DT[x_bf16])
    x32, x64 = x.float(), x.double()
    pa = torch.rand(C, generator=_gen(2)) + 0.5
    pd = torch.randn(C, generator=_gen(3))
    xd, pad, pdd = dev(x, DT[x_bf16]), dev(pa), dev(pd)
    for wide in (0, 1):
        stride, off = _rows(N, CHW, wide)
        out = Buf(N * stride)
        for affine in (0, 1):
            for slope in (1.0, 0.0, 0.2):
                for by_ptr in (0, 1):
                    sp = torch.tensor([slope], device='cuda') if by_ptr else None
                    run2(lambda: lib.sisr_nhwc_to_nchw(xd.data_ptr(), pad.data_ptr() if affine else None,
                                                       pdd.data_ptr() if affine else None, sp.data_ptr() if by_ptr else None,
                                                       7.0 if by_ptr else slope, out.ptr(off), stride, N, H, W, C, x_bf16, _st()),
                         [out])
                    rows = out.cpu().view(N, stride)
                    assert bool((rows[:, :off] == SENT).all()) and bool((rows[:, off + CHW:] == SENT).all()), 'gap overwritten'
                    got = rows[:, off:off + CHW].reshape(N, C, H, W)
                    what = 'nhwc_to_nchw %s wide=%d affine=%d slope=%g ptr=%d' % (shape, wide, affine, slope, by_ptr)
                    if not affine:              # movement and one fp32 multiply: bit-exact
                        s32 = torch.tensor(slope, dtype=F32)
                        ref = torch.where(x32 > 0, x32, s32 * x32).permute(0, 3, 1, 2)
                        assert torch.equal(got, ref), what
                    else:                       # pa * x + pd may be fused: terms |pa x| and |pd|
                        v = pa.double() * x64 + pd.double()
                        terms = (pa.double() * x64).abs() + pd.double().abs()
                        assert_within(got, lrelu64(v, slope).permute(0, 3, 1, 2), (2 * U * terms).permute(0, 3, 1, 2), what)


@pytest.mark.parametrize('y_bf16', [0, 1])
@pytest.mark.parametrize('shape', T_SHAPES)
def test_nchw_to_nhwc(lib, shape, y_bf16):
    N, H, W, C = shape
    CHW = C * H * W
    x = torch.randn(N, C, H, W, generator=_gen(4))
    ref = x.permute(0, 2, 3, 1).contiguous().to(DT[y_bf16])
    for wide in (0, 1):
        stride, off = _rows(N, CHW, wide)
        src = torch.full((N, stride), float('nan'))          # a read outside the slot would bring a NaN
        src[:, off:off + CHW] = x.reshape(N, CHW)
        srcd = src.cuda()
        out = Buf(N * CHW, DT[y_bf16])
        run2(lambda: lib.sisr_nchw_to_nhwc(srcd.data_ptr() + 4 * off, stride, out.ptr(), N, H, W, C, y_bf16, _st()), [out])
        assert torch.equal(out.cpu().view(N, H, W, C), ref), (shape, wide)


# ---- NCHW gradient image -> NHWC padded to 4 channels, tanh backward fused -------------------------------------------------------
def _grad_to_nhwc4(lib, N, C, H, W, Cpad, with_out):
    dy = torch.randn(N, C, H, W, generator=_gen(5))
    y = torch.tanh(1.5 * torch.randn(N, C, H, W, generator=_gen(6)))
    dyd, yd = dev(dy), dev(y)
    g = Buf(N * H * W * Cpad, fill=float('nan'))
    run2(lambda: lib.sisr_nchw_grad_to_nhwc4(dyd.data_ptr(), yd.data_ptr() if with_out else None, g.ptr(), N, C, H, W, Cpad,
                                             _st()), [g])
    got = g.cpu().view(N, H, W, Cpad)
    assert bool((got[..., C:] == 0).all()), 'padding channels must be exactly 0'
    got = got[..., :C].permute(0, 3, 1, 2)
    if not with_out:
        assert torch.equal(got, dy)
    else:           # dy * (1 - y^2): terms |dy| and |dy y^2| -- an absolute bound, 1 - y^2 cancels near |y| = 1
        d, t = dy.double(), y.double()
        assert_within(got, d * (1 - t * t), 2 * U * (d.abs() + (d * t * t).abs()), 'nchw_grad_to_nhwc4 C=%d Cpad=%d' % (C, Cpad))


@pytest.mark.parametrize('with_out', [0, 1])
@pytest.mark.parametrize('C,Cpad', [(3, 4), (1, 4), (5, 8), (3, 8)])
def test_nchw_grad_to_nhwc4(lib, C, Cpad, with_out):
    _grad_to_nhwc4(lib, 2, C, 5, 7, Cpad, with_out)


def test_nchw_grad_to_nhwc4_past_grid_cap(lib):
    """cap 4096 x 256 = 1,048,576 pixels per trip: 1025 x 1024 = 1,049,600 pixels take a second trip"""
    assert 1025 * 1024 > 4096 * 256
    _grad_to_nhwc4(lib, 1, 3, 1025, 1024, 4, 1)


# ---- 2x2 max-pool forward, fused ReLU + pool backward ---------------------------------------------------------------------------
POOL_GRID = torch.tensor([-2.0, -1.0, -0.5, -0.25, 0.0, 0.0, 0.5, 1.0])      # exact in bf16; zeros and positives repeat


def _pool_input(N, C, H, W, seed):
    return POOL_GRID[torch.randint(0, 8, (N, C, H, W), generator=_gen(seed))]


def _window_classes(x):
    """(all < 0, maximum exactly 0, unique positive maximum, tied positive maximum) counts over the 2x2 windows of x (NCHW)"""
    N, C, H, W = x.shape
    Ho, Wo = H // 2, W // 2
    w = x[:, :, :2 * Ho, :2 * Wo].reshape(N, C, Ho, 2, Wo, 2).permute(0, 1, 2, 4, 3, 5).reshape(-1, 4)
    mx = w.max(dim=1).values
    ties = (w == mx[:, None]).sum(dim=1)
    return (int((mx < 0).sum()), int((mx == 0).sum()), int(((mx > 0) & (ties == 1)).sum()), int(((mx > 0) & (ties > 1)).sum()))


def _pool_fwd_bwd(lib, N, C, H, W, bf16):
    dt = DT[bf16]
    Ho, Wo = H // 2, W // 2
    x = _pool_input(N, C, H, W, 7)
    classes = _window_classes(x)
    assert all(c > 0 for c in classes), classes               # every window class is present in this very input
    dy = torch.randn(N, C, Ho, Wo, generator=_gen(8)).to(dt).float()
    xr = x.clone().requires_grad_(True)
    F.max_pool2d(F.relu(xr), 2, 2).backward(dy)               # torch: first maximum of the window, ReLU gate x > 0
    ref_y = F.max_pool2d(x, 2, 2).permute(0, 2, 3, 1).contiguous().to(dt)     # the kernel pools the raw map
    ref_dx = xr.grad.permute(0, 2, 3, 1).contiguous().to(dt)
    xd = dev(x.permute(0, 2, 3, 1), dt)
    dyd = dev(dy.permute(0, 2, 3, 1), dt)
    y, dx = Buf(N * Ho * Wo * C, dt), Buf(N * H * W * C, dt)
    run2(lambda: lib.sisr_maxpool2_fwd(xd.data_ptr(), y.ptr(), N, H, W, C, 3 if bf16 else 0, _st()), [y])
    assert torch.equal(y.cpu().view(N, Ho, Wo, C), ref_y), 'pool forward'
    run2(lambda: lib.sisr_maxpool2_relu_bwd(dyd.data_ptr(), xd.data_ptr(), dx.ptr(), N, H, W, C, 7 if bf16 else 0, _st()), [dx])
    got = dx.cpu().view(N, H, W, C)
    if H & 1:
        assert bool((got[:, H - 1] == 0).all()), 'uncovered last row must be exactly 0'
    if W & 1:
        assert bool((got[:, :, W - 1] == 0).all()), 'uncovered last column must be exactly 0'
    assert torch.equal(got, ref_dx), 'pool backward'


@pytest.mark.parametrize('bf16', [0, 1])
@pytest.mark.parametrize('C', [4, 8, 64])
@pytest.mark.parametrize('H,W', [(2, 2), (7, 5), (6, 9), (9, 6), (12, 12)])
def test_maxpool2_fwd_and_relu_bwd(lib, H, W, C, bf16):
    N = max(2, math.ceil(160 / ((H // 2) * (W // 2) * C)))    # >= 160 windows: all four classes turn up (asserted)
    _pool_fwd_bwd(lib, N, C, H, W, bf16)


@pytest.mark.parametrize('bf16', [0, 1])
def test_maxpool2_past_grid_cap_odd_map(lib, bf16):
    """cap 4096 x 256 = 1,048,576 (pooled pixel, 4 channels) items per trip: 257 x 257 x 16 = 1,056,784 take a second trip; H and W
    odd, so the edge kernel (1024 x 256 threads, also looping) zeroes a row and a column of the 515 x 515 x 64 map (68 MB fp32)"""
    assert 257 * 257 * 16 > 4096 * 256
    _pool_fwd_bwd(lib, 1, 64, 515, 515, bf16)


@pytest.mark.parametrize('H,W,C', [(7, 5, 8), (6, 9, 4), (12, 12, 64)])
def test_maxpool2_fwd_mixed_storage(lib, H, W, C):
    """dt = 1 (bf16 in, fp32 out) and dt = 2 (fp32 in, bf16 out): compiled and exported, not reached from the engine"""
    N, Ho, Wo = 3, H // 2, W // 2
    x = torch.randn(N, C, H, W, generator=_gen(9))
    for dt in (1, 2):
        xs = x.to(DT[dt & 1])
        ref = F.max_pool2d(xs.float(), 2, 2).permute(0, 2, 3, 1).contiguous().to(DT[dt >> 1])
        xd = dev(xs.permute(0, 2, 3, 1), DT[dt & 1])
        y = Buf(N * Ho * Wo * C, DT[dt >> 1])
        run2(lambda: lib.sisr_maxpool2_fwd(xd.data_ptr(), y.ptr(), N, H, W, C, dt, _st()), [y])
        assert torch.equal(y.cpu().view(N, Ho, Wo, C), ref), dt


def test_maxpool2_relu_bwd_refuses_mixed_storage(lib):
    t = torch.zeros(2 * 4 * 4 * 8, device='cuda')
    for dt in range(1, 7):
        assert lib.sisr_maxpool2_relu_bwd(t.data_ptr(), t.data_ptr(), t.data_ptr(), 2, 4, 4, 8, dt, _st()) == UNSUPPORTED


# ---- element-wise -------------------------------------------------------------------------------------------------------------
def _with_zeros(t, seed, frac=0.2):
    t = t.clone()
    t[torch.rand(t.shape, generator=_gen(seed)) < frac] = 0.0
    return t


# cap 4096 x 256 = 1,048,576 elements per trip
@pytest.mark.parametrize('n', [1, 255, 4097, 4096 * 256 + 257])
def test_add_relu_masked(lib, n):
    a = torch.randn(n, generator=_gen(10))
    b = torch.randn(n, generator=_gen(11))
    ref = _with_zeros(torch.randn(n, generator=_gen(12)), 13)
    assert n < 4 or bool((ref == 0).any())
    host = {k: {bf: t.to(DT[bf]) for bf in (0, 1)} for k, t in (('a', a), ('b', b), ('r', ref))}
    devs = {k: {bf: dev(v[bf], DT[bf]) for bf in (0, 1)} for k, v in host.items()}
    outs = {bf: Buf(n, DT[bf]) for bf in (0, 1)}
    for dt in range(16):
        ab, bb, rb, ob = dt & 1, (dt >> 1) & 1, (dt >> 2) & 1, (dt >> 3) & 1
        for a_null in (0, 1):
            out = outs[ob]
            run2(lambda: lib.sisr_add_relu_masked(None if a_null else devs['a'][ab].data_ptr(), devs['b'][bb].data_ptr(),
                                                  devs['r'][rb].data_ptr(), out.ptr(), n, dt, _st()), [out])
            m = torch.where(host['r'][rb].float() > 0, host['b'][bb].float(), torch.zeros(()))
            want = (m if a_null else host['a'][ab].float() + m).to(DT[ob])       # one fp32 addition: exact
            assert torch.equal(out.cpu(), want), (n, dt, a_null)


# cap 2048 x 256 = 524,288 elements per trip
@pytest.mark.parametrize('n', [3, 2048 * 256 + 3])
def test_act_bwd(lib, n):
    dy = torch.randn(n, generator=_gen(14))
    dyd = dev(dy)
    out = Buf(n)
    # kind 0: LeakyReLU backward, gate on the saved activation (exact zeros take the slope branch)
    ref = _with_zeros(torch.randn(n, generator=_gen(15)), 16)
    ref[0] = 0.0
    refd = dev(ref)
    for slope in (0.2, 0.0):
        run2(lambda: lib.sisr_act_bwd(dyd.data_ptr(), refd.data_ptr(), out.ptr(), n, 0, slope, _st()), [out])
        want = torch.where(ref > 0, dy, torch.tensor(slope, dtype=F32) * dy)
        assert torch.equal(out.cpu(), want), (n, slope)
    # kind 1: sigmoid backward dy * r * (1 - r) = dy r - dy r^2 (the terms), r = a saved sigmoid.  Three roundings: dy r, 1 - r, the
    # product.  For r in [1/8, 1]: |err| <= 2u |dy r (1 - r)| + |dy r| u / 2  (1 - r <= 1: its half-ulp is u / 2)
    #                                    <= 2u |dy r| (1 - r + 1/4) <= 2u |dy r| (1 + r)  since r >= 1/8;  r = 0 gives an exact 0.
    r = 0.125 + 0.875 * torch.rand(n, generator=_gen(17))
    r = _with_zeros(r, 18)
    r[0], r[n - 1] = 0.0, 1.0
    rd = dev(r)
    run2(lambda: lib.sisr_act_bwd(dyd.data_ptr(), rd.data_ptr(), out.ptr(), n, 1, 0.0, _st()), [out])
    d, q = dy.double(), r.double()
    assert_within(out.cpu(), d * q * (1 - q), 2 * U * ((d * q).abs() + (d * q * q).abs()), 'act_bwd kind 1 n=%d' % n)
    assert bool((out.cpu()[r == 0] == 0).all())


# cap 4096 x 256 = 1,048,576 float4 per trip; the n & 3 tail is done by workgroup 0
@pytest.mark.parametrize('n', [1, 2, 3, 5, 6, 7, 1027, 4 * (4096 * 256 + 37) + 3])
def test_add(lib, n):
    a = torch.randn(n, generator=_gen(19))
    b = torch.randn(n, generator=_gen(20))
    for dt in (0, 7, 4):
        di, do = DT[dt & 1], DT[dt >> 2]
        ah, bh = a.to(di), b.to(di)
        ad, bd = dev(ah, di), dev(bh, di)
        y = Buf(n, do)
        run2(lambda: lib.sisr_add(ad.data_ptr(), bd.data_ptr(), y.ptr(), n, dt, _st()), [y])
        assert torch.equal(y.cpu(), (ah.float() + bh.float()).to(do)), (n, dt)
    t = torch.zeros(16, device='cuda')
    for dt in (1, 2, 3, 5, 6):
        assert lib.sisr_add(t.data_ptr(), t.data_ptr(), t.data_ptr(), 16, dt, _st()) == UNSUPPORTED


def _eltwise(lib, P, C, dt, x2_mode, by_ptr, slope=0.25):
    """y = lrelu(x1, slope) [+ x2 | + pa[c] x2 + pd[c]];  dt bit 0 / 1 / 2: x1 / x2 / y stored as bf16"""
    x1 = torch.randn(P, C, generator=_gen(21)).to(DT[dt & 1])
    x2 = torch.randn(P, C, generator=_gen(22)).to(DT[(dt >> 1) & 1])
    pa = torch.rand(C, generator=_gen(23)) + 0.5
    pd = torch.randn(C, generator=_gen(24))
    x1d, x2d, pad, pdd = dev(x1, x1.dtype), dev(x2, x2.dtype), dev(pa), dev(pd)
    sp = torch.tensor([slope], device='cuda')
    y = Buf(P * C, DT[(dt >> 2) & 1])
    run2(lambda: lib.sisr_eltwise_res_affine(x1d.data_ptr(), sp.data_ptr() if by_ptr else None, 7.0 if by_ptr else slope,
                                             x2d.data_ptr() if x2_mode else None, pad.data_ptr() if x2_mode == 2 else None,
                                             pdd.data_ptr() if x2_mode == 2 else None, y.ptr(), P, C, dt, _st()), [y])
    r = lrelu64(x1.double(), slope)
    terms = r.abs()
    if x2_mode == 1:
        r, terms = r + x2.double(), terms + x2.double().abs()
    elif x2_mode == 2:
        r = r + pa.double() * x2.double() + pd.double()
        terms = terms + (pa.double() * x2.double()).abs() + pd.double().abs()
    bound = 2 * U * terms + (2.0 ** -8 * r.abs() if dt & 4 else 0.0)
    assert_within(y.cpu().view(P, C), r, bound, 'eltwise P=%d C=%d dt=%d x2=%d ptr=%d' % (P, C, dt, x2_mode, by_ptr))


@pytest.mark.parametrize('C', [4, 12, 24, 64, 128])
def test_eltwise_res_affine(lib, C):
    """all 8 storage keys; C = 64 / 128 with dt = 7 take the bf16x8 kernel, C = 24 (8 | C, but C does not divide 2048) falls back"""
    for dt in range(8):
        for x2_mode in (0, 1, 2):
            for by_ptr in (0, 1):
                _eltwise(lib, 37, C, dt, x2_mode, by_ptr)


# generic kernel: cap 4096 x 256 = 1,048,576 float4 per trip -> C = 64: P > 65,536; C = 24: P > 174,762 (its stride of 2^22
#   elements is NOT a multiple of 24: the channel of a thread changes from trip to trip)
# bf16x8 kernel: cap 2048 x 256 = 524,288 octets per trip -> C = 64: P > 65,536
@pytest.mark.parametrize('C,P,dt,x2_mode', [(64, 65600, 0, 2), (64, 65600, 7, 2), (64, 65600, 7, 1), (24, 180000, 0, 2),
                                            (24, 180000, 7, 2)])
def test_eltwise_res_affine_past_grid_cap(lib, C, P, dt, x2_mode):
    assert P * C // 4 > 4096 * 256 and P * C // 8 > 2048 * 256
    _eltwise(lib, P, C, dt, x2_mode, 1)


@pytest.mark.parametrize('n', [5, 8192, 3 * 8192 + 5])
def test_prelu_slope_grad(lib, n):
    """out = sum over !(pre > 0) of dy * pre.  D = 54: a thread adds at most 8 float4 = 32 products and one tail element (33),
    wave_sum 6 levels, 4 wave totals through LDS (4); sum_partials: 1 partial per thread (<= 256 workgroups), 6 + 4 again (11)"""
    D = 33 + 6 + 4 + 1 + 6 + 4
    dy0 = torch.randn(n, generator=_gen(25))
    pre0 = _with_zeros(torch.randn(n, generator=_gen(26)), 27)
    pre0[0] = 0.0
    blocks = min((n + 8191) // 8192, 1024)
    for dt in range(4):
        dy, pre = dy0.to(DT[dt & 1]), pre0.to(DT[dt >> 1])
        dyd, pred = dev(dy, dy.dtype), dev(pre, pre.dtype)
        work, out = Buf(blocks), Buf(1)
        run2(lambda: lib.sisr_prelu_slope_grad(dyd.data_ptr(), pred.data_ptr(), n, work.ptr(), out.ptr(), dt, _st()), [work, out])
        prod = (dy.double() * pre.double())[~(pre.float() > 0)]
        assert_within(out.cpu(), prod.sum().reshape(1), (2 * D * U * prod.abs().sum()).reshape(1), 'prelu_slope_grad n=%d dt=%d' % (n, dt))


# ---- generic fully connected ----------------------------------------------------------------------------------------------------
def _fc_rows_per_split(K, Nout):
    """layout_fc.hip: enough (K block, Nout split) workgroups for 512, at most 256 rows per split"""
    blocks_k = ((K >> 2) + 255) // 256
    splits = max(1, min(Nout, (512 + blocks_k - 1) // blocks_k))
    rows = (Nout + splits - 1) // splits
    return min(rows, 256), rows


FC_CASES = [(1, 4, 1), (5, 36, 7), (16, 4100, 1), (13, 2052, 130),
            # split reduce: cap 2048 x 256 = 524,288 float4 per trip; 16 x 131200 / 4 = 524,800
            (16, 131200, 8),
            # Nout K = 2^27 + 2^19 > 2^27: 2 splits of 257 rows are cut to 256 rows -> 3 splits, the last of 2 rows
            (16, 262144, 514)]


@pytest.mark.parametrize('B,K,Nout', FC_CASES)
def test_fc_forward_dgrad_wgrad(lib, B, K, Nout):
    big = Nout * K > 1 << 20                   # the two large cases: float64 references formed on the device
    where = 'cuda' if big else 'cpu'
    x = torch.randn(B, K, generator=_gen(28))
    Wt = torch.randn(Nout, K, generator=_gen(29)) * K ** -0.5
    bias = torch.randn(Nout, generator=_gen(30))
    dy = torch.randn(B, Nout, generator=_gen(31))
    xd, Wd, bd, dyd = dev(x), dev(Wt), dev(bias), dev(dy)
    W64 = (Wd if big else Wt).double()
    x64, dy64, b64 = x.double().to(where), dy.double().to(where), bias.double().to(where)

    def fetch(buf):
        return buf.body if big else buf.cpu()

    # forward.  D = 4 ceil(K / 1024) + 10: a thread adds ceil(K / 1024) float4 dot products of 4 terms into its accumulator, wave_sum
    # 6 levels, 3 additions over the waves, 1 for the bias.  Sigmoid epilogue: |sigma'| <= 1/4 on the bound of the sum, plus expf,
    # 1 + e and the division at one ulp (2^-23) each of a result <= 1, rounded up to 8u.
    D = 4 * ((K + 1023) // 1024) + 10
    y = Buf(B * Nout)
    for in_slope in (1.0, 0.01):
        xa = lrelu64(x64, in_slope)
        for with_bias in (0, 1):
            ref = xa @ W64.t() + (b64 if with_bias else 0.0)
            terms = xa.abs() @ W64.abs().t() + (b64.abs() if with_bias else 0.0)
            for epi in (0, 1):
                run2(lambda: lib.sisr_fc_forward(xd.data_ptr(), in_slope, Wd.data_ptr(), bd.data_ptr() if with_bias else None,
                                                 y.ptr(), B, K, Nout, epi, _st()), [y])
                what = 'fc_forward %s slope=%g bias=%d epi=%d' % ((B, K, Nout), in_slope, with_bias, epi)
                if epi == 0:
                    assert_within(fetch(y).view(B, Nout), ref, 2 * D * U * terms, what)
                else:
                    assert_within(fetch(y).view(B, Nout), torch.sigmoid(ref), 0.25 * 2 * D * U * terms + 8 * U, what)
    del y

    # data gradient.  D = rows + splits: one fused multiply-add per weight row of the split, then the splits are added in order
    rows, rows_uncapped = _fc_rows_per_split(K, Nout)
    splits = lib.sisr_fc_dgrad_splits(K, Nout)
    assert splits == (Nout + rows - 1) // rows
    if (B, K, Nout) == FC_CASES[-1]:
        assert rows_uncapped > 256 and splits == 3             # the 256-row cap is what sets the split count here
    dx, work = Buf(B * K), Buf((splits + 1) * B * K)
    run2(lambda: lib.sisr_fc_dgrad(dyd.data_ptr(), Wd.data_ptr(), dx.ptr(), work.ptr(), B, K, Nout, _st()), [dx, work])
    slices = work.body.view(splits + 1, B * K)
    assert not bool((slices[:splits] == SENT).any()), 'a slice of work the split count promises was not written'
    assert bool((slices[splits] == SENT).all()), 'more slices of work written than sisr_fc_dgrad_splits says'
    assert_within(fetch(dx).view(B, K), dy64 @ W64, 2 * (rows + splits) * U * (dy64.abs() @ W64.abs()), 'fc_dgrad %s' % ((B, K, Nout),))
    del dx, work, slices

    # weight gradient: D = 16, one fused multiply-add per batch row (rows past B are zeros); bias gradient: D = B
    dW, db = Buf(Nout * K), Buf(Nout)
    for in_slope in (1.0, 0.01):
        xa = lrelu64(x64, in_slope)
        ref_w, bound_w = dy64.t() @ xa, 2 * 16 * U * (dy64.abs().t() @ xa.abs())
        for with_db in (0, 1):
            run2(lambda: lib.sisr_fc_wgrad(dyd.data_ptr(), xd.data_ptr(), in_slope, dW.ptr(), db.ptr() if with_db else None,
                                           B, K, Nout, _st()), [dW, db])
            what = 'fc_wgrad %s slope=%g db=%d' % ((B, K, Nout), in_slope, with_db)
            assert_within(fetch(dW).view(Nout, K), ref_w, bound_w, what)
            if with_db:
                assert_within(fetch(db), dy64.sum(dim=0), 2 * B * U * dy64.abs().sum(dim=0), what + ' db')
            else:
                assert bool((db.body == SENT).all()), 'db written although null was passed'


# ---- BatchNorm constants --------------------------------------------------------------------------------------------------------
def _bn_partials(counts, C, seed):
    """per-tile (count, mean, M2) of a random (P, C) tensor cut into tiles of the given sizes, rounded to fp32 as the producing
    kernels store them; every channel has a positive mean, channel C-1 a mean of 100 with sigma 0.01"""
    g = _gen(seed)
    P = int(sum(counts))
    mu = 0.5 + 1.5 * torch.rand(C, generator=g, dtype=torch.float64)
    sd = 0.5 + torch.rand(C, generator=g, dtype=torch.float64)
    mu[C - 1], sd[C - 1] = 100.0, 0.01
    data = (torch.randn(P, C, generator=g, dtype=torch.float64) * sd + mu).float().double()
    stat = np.zeros((len(counts), 2, C), dtype=np.float32)
    at = 0
    for t, n in enumerate(counts):
        tile = data[at:at + n]
        m = tile.mean(dim=0)
        stat[t, 0] = m.numpy()
        stat[t, 1] = ((tile - m) ** 2).sum(dim=0).numpy()
        at += n
    return stat, np.asarray(counts, dtype=np.float32)


def _chan_merge(stat, cnt):
    """float64 pairwise update of Chan et al. over the fp32-rounded partials, tile by tile"""
    n, mean, m2 = 0.0, np.zeros(stat.shape[2]), np.zeros(stat.shape[2])
    for t in range(stat.shape[0]):
        nb, mb, qb = float(cnt[t]), stat[t, 0].astype(np.float64), stat[t, 1].astype(np.float64)
        d = mb - mean
        tot = n + nb
        mean = mean + d * (nb / tot)
        m2 = m2 + qb + d * d * (n * nb / tot)
        n = tot
    return n, mean, m2


def _bn_finalize(lib, counts, C, seed):
    stat, cnt = _bn_partials(counts, C, seed)
    g = _gen(seed + 1)
    gamma = (0.5 + torch.rand(C, generator=g)).numpy()
    beta = (-0.2 - 0.8 * torch.rand(C, generator=g)).numpy()        # shift = beta - mean * scale: both parts negative, no cancellation
    rm0 = (0.5 + torch.rand(C, generator=g)).numpy()
    rv0 = (0.5 + torch.rand(C, generator=g)).numpy()
    mom, eps = float(np.float32(0.1)), float(np.float32(1e-5))
    statd, cntd = torch.from_numpy(stat).cuda(), torch.from_numpy(cnt).cuda()
    gd, bd = torch.from_numpy(gamma).cuda(), torch.from_numpy(beta).cuda()
    rm, rv = Buf(C), Buf(C)
    outs = [Buf(C) for _ in range(4)]

    def call():
        rm.body.copy_(torch.from_numpy(rm0))                        # the running statistics are updated in place
        rv.body.copy_(torch.from_numpy(rv0))
        return lib.sisr_bn_finalize(statd.data_ptr(), cntd.data_ptr(), len(counts), C, gd.data_ptr(), bd.data_ptr(), rm.ptr(),
                                    rv.ptr(), mom, eps, outs[0].ptr(), outs[1].ptr(), outs[2].ptr(), outs[3].ptr(), _st())
    run2(call, [rm, rv] + outs)
    n, mean, m2 = _chan_merge(stat, cnt)
    var = m2 / n
    invstd = 1.0 / np.sqrt(var + eps)
    scale = gamma.astype(np.float64) * invstd
    shift = beta.astype(np.float64) - mean * scale
    unb = m2 / (n - 1.0) if n > 1 else var                          # a single sample: the biased value
    what = 'bn_finalize tiles=%d C=%d' % (len(counts), C)
    for name, buf, ref in (('scale', outs[0], scale), ('shift', outs[1], shift), ('mean', outs[2], mean), ('invstd', outs[3], invstd)):
        ref = torch.from_numpy(ref)
        assert_within(buf.cpu(), ref, 4 * U * ref.abs(), what + ' ' + name)
    # running statistics: 4u (|old| + |new|).  "new" is read both ways -- the batch statistic and the updated running value -- and the
    # smaller of the two bounds is applied (the kernel's error is three fp32 roundings: 1 - m, the cast of the statistic, the fma)
    for name, buf, old, new in (('running_mean', rm, rm0, mean), ('running_var', rv, rv0, unb)):
        old64, new64 = torch.from_numpy(old).double(), torch.from_numpy(np.asarray(new, dtype=np.float64))
        upd = (1.0 - mom) * old64 + mom * new64
        bound = 4 * U * (old64.abs() + torch.minimum(new64.abs(), upd.abs()))
        assert_within(buf.cpu(), upd, bound, what + ' ' + name)


def _uneven_counts(n_tiles, seed):
    c = torch.randint(1, 10, (n_tiles,), generator=_gen(seed)).tolist()
    c[0] = 1                                                        # a tile of a single sample (its M2 is 0)
    if n_tiles > 1:
        c[-1] = 23
    return c


# 256 tile-splits per channel: 1 tile, fewer tiles than splits, exactly 256, one more, several per split
@pytest.mark.parametrize('C', [3, 4, 64, 130])                      # C % 4 != 0: the last workgroup clamps its channel index
@pytest.mark.parametrize('n_tiles', [1, 3, 255, 256, 257, 700])
def test_bn_finalize(lib, n_tiles, C):
    counts = _uneven_counts(n_tiles, 40 + n_tiles)
    if n_tiles == 1:
        _bn_finalize(lib, [37], C, 50)                              # one tile of several samples ...
    _bn_finalize(lib, counts, C, 60 + C)                            # ... (n_tiles == 1: one sample in all: variance 0, unbiased = biased)


@pytest.mark.parametrize('C', [1, 3, 64, 257])
def test_bn_eval_consts(lib, C):
    """scale = gamma / sqrtf(rv + eps): the addition, the square root (halved) and the division at u each: 4u relative with room.
    shift = beta - rm * scale (possibly fused): the error of scale carried by rm * scale plus one or two roundings:
    4u (|beta| + |rm scale|)."""
    g = _gen(70 + C)
    gamma, beta, rm = (torch.randn(C, generator=g) for _ in range(3))
    rv = 0.05 + torch.rand(C, generator=g)
    eps = float(np.float32(1e-5))
    sc, sh = Buf(C), Buf(C)
    ins = [dev(t) for t in (gamma, beta, rm, rv)]
    run2(lambda: lib.sisr_bn_eval_consts(ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), ins[3].data_ptr(), eps, C,
                                         sc.ptr(), sh.ptr(), _st()), [sc, sh])
    scale = gamma.double() / torch.sqrt(rv.double() + eps)
    assert_within(sc.cpu(), scale, 4 * U * scale.abs(), 'bn_eval_consts scale C=%d' % C)
    assert_within(sh.cpu(), beta.double() - rm.double() * scale, 4 * U * (beta.double().abs() + (rm.double() * scale).abs()),
                  'bn_eval_consts shift C=%d' % C)
