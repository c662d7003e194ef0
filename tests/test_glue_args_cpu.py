"""CPU: argument rejection of the glue entry points (layout, pooling, element-wise, generic FC, BatchNorm constants).

Every case below is read off the wrapper's source (csrc/layout_fc.hip, csrc/norm.hip): the argument set fails a check that
sits BEFORE the first hipLaunchKernelGGL, so the call returns SISR_E_BADARG / SISR_E_UNSUPPORTED without touching a device and
the pointers (made-up addresses) are never dereferenced.  tests/test_gpu_glue.py holds the value tests of the same entry points."""
import importlib

import pytest

BADARG, UNSUPPORTED = -1, -3            # include/sisr_hip.h
P = 0x10000                             # a made-up, 16-byte aligned, non-null device address
Q = P + 4                               # the same, not 16-byte aligned
NUL = None


@pytest.fixture(scope='module')
def lib():
    return importlib.import_module('single-image-super-resolution_amd._lib').lib()


def _cases():
    c = []

    def add(fn, want, what, *args):
        c.append(pytest.param(fn, want, args, id='%s-%s' % (fn[5:], what)))

    # sisr_maxpool2_fwd(x, y, N, H, W, C, dt, stream)
    ok = [P, P, 2, 6, 6, 8, 0, NUL]
    for what, i, v in (('null_x', 0, NUL), ('null_y', 1, NUL), ('N0', 2, 0), ('H1', 3, 1), ('W1', 4, 1), ('C0', 5, 0),
                       ('C_and_3', 5, 6)):
        add('sisr_maxpool2_fwd', BADARG, what, *(ok[:i] + [v] + ok[i + 1:]))
    # sisr_maxpool2_relu_bwd(dy, x, dx, N, H, W, C, dt, stream)
    ok = [P, P, P, 2, 6, 6, 8, 0, NUL]
    for what, i, v in (('null_dy', 0, NUL), ('null_x', 1, NUL), ('null_dx', 2, NUL), ('N0', 3, 0), ('H1', 4, 1), ('W1', 5, 1),
                       ('C_and_3', 6, 10)):
        add('sisr_maxpool2_relu_bwd', BADARG, what, *(ok[:i] + [v] + ok[i + 1:]))
    for dt in range(1, 7):                                            # all fp32 (0) or all bf16 (7) only
        add('sisr_maxpool2_relu_bwd', UNSUPPORTED, 'mixed_dt%d' % dt, *(ok[:7] + [dt, NUL]))
    # sisr_add_relu_masked(a, b, ref, out, n, dt, stream): a may be null
    ok = [P, P, P, P, 100, 0, NUL]
    for what, i, v in (('null_b', 1, NUL), ('null_ref', 2, NUL), ('null_out', 3, NUL), ('n0', 4, 0), ('n_neg', 4, -5)):
        add('sisr_add_relu_masked', BADARG, what, *(ok[:i] + [v] + ok[i + 1:]))
    # sisr_nhwc_to_nchw(x, pa, pd, slope_p, slope, y, dst_stride, N, H, W, C, x_bf16, stream)
    ok = [P, NUL, NUL, NUL, 1.0, P, 3 * 5 * 7, 2, 5, 7, 3, 0, NUL]
    for what, i, v in (('null_x', 0, NUL), ('null_y', 5, NUL), ('pa_without_pd', 1, P), ('short_stride', 6, 3 * 5 * 7 - 1),
                       ('N0', 7, 0), ('H0', 8, 0), ('W0', 9, 0), ('C0', 10, 0)):
        add('sisr_nhwc_to_nchw', BADARG, what, *(ok[:i] + [v] + ok[i + 1:]))
    # sisr_nchw_to_nhwc(x, src_stride, y, N, H, W, C, y_bf16, stream)
    ok = [P, 3 * 5 * 7, P, 2, 5, 7, 3, 0, NUL]
    for what, i, v in (('null_x', 0, NUL), ('null_y', 2, NUL), ('short_stride', 1, 3 * 5 * 7 - 1), ('N0', 3, 0), ('C0', 6, 0)):
        add('sisr_nchw_to_nhwc', BADARG, what, *(ok[:i] + [v] + ok[i + 1:]))
    # sisr_nchw_grad_to_nhwc4(dy, out, g, N, C, H, W, Cpad, stream): out may be null
    ok = [P, NUL, P, 2, 3, 5, 7, 4, NUL]
    for what, i, v in (('null_dy', 0, NUL), ('null_g', 2, NUL), ('Cpad_lt_C', 4, 5), ('Cpad_and_3', 7, 6), ('N0', 3, 0),
                       ('H0', 5, 0), ('W0', 6, 0), ('C0', 4, 0)):
        add('sisr_nchw_grad_to_nhwc4', BADARG, what, *(ok[:i] + [v] + ok[i + 1:]))
    # sisr_fc_forward(x, in_slope, W, bias, y, B, K, Nout, epi, stream): bias may be null
    ok = [P, 1.0, P, NUL, P, 4, 36, 7, 0, NUL]
    for what, i, v in (('null_x', 0, NUL), ('null_W', 2, NUL), ('null_y', 4, NUL), ('B0', 5, 0), ('B17', 5, 17), ('K0', 6, 0),
                       ('K_and_3', 6, 38), ('Nout0', 7, 0)):
        add('sisr_fc_forward', BADARG, what, *(ok[:i] + [v] + ok[i + 1:]))
    # sisr_fc_dgrad(dy, W, dx, work, B, K, Nout, stream)
    ok = [P, P, P, P, 4, 36, 7, NUL]
    for what, i, v in (('null_dy', 0, NUL), ('null_W', 1, NUL), ('null_dx', 2, NUL), ('null_work', 3, NUL), ('B0', 4, 0),
                       ('B17', 4, 17), ('K_and_3', 5, 37), ('Nout0', 6, 0)):
        add('sisr_fc_dgrad', BADARG, what, *(ok[:i] + [v] + ok[i + 1:]))
    # sisr_fc_wgrad(dy, x, in_slope, dW, db, B, K, Nout, stream): db may be null
    ok = [P, P, 1.0, P, NUL, 4, 36, 7, NUL]
    for what, i, v in (('null_dy', 0, NUL), ('null_x', 1, NUL), ('null_dW', 3, NUL), ('B0', 5, 0), ('B17', 5, 17),
                       ('K_and_3', 6, 39), ('Nout0', 7, 0)):
        add('sisr_fc_wgrad', BADARG, what, *(ok[:i] + [v] + ok[i + 1:]))
    # sisr_act_bwd(dy, ref, out, n, kind, slope, stream)
    ok = [P, P, P, 100, 0, 0.2, NUL]
    for what, i, v in (('null_dy', 0, NUL), ('null_ref', 1, NUL), ('null_out', 2, NUL), ('n0', 3, 0), ('kind2', 4, 2),
                       ('kind_neg', 4, -1)):
        add('sisr_act_bwd', BADARG, what, *(ok[:i] + [v] + ok[i + 1:]))
    # sisr_bn_finalize(stat, cnt, n_tiles, C, gamma, beta, rm, rv, momentum, eps, scale, shift, mean, invstd, stream)
    ok = [P, P, 3, 8, P, P, P, P, 0.1, 1e-5, P, P, P, P, NUL]
    for i in (0, 1, 4, 5, 6, 7, 10, 11, 12, 13):
        add('sisr_bn_finalize', BADARG, 'null_arg%d' % i, *(ok[:i] + [NUL] + ok[i + 1:]))
    add('sisr_bn_finalize', BADARG, 'n_tiles0', *(ok[:2] + [0] + ok[3:]))
    add('sisr_bn_finalize', BADARG, 'C0', *(ok[:3] + [0] + ok[4:]))
    # sisr_bn_eval_consts(gamma, beta, rm, rv, eps, C, scale, shift, stream)
    ok = [P, P, P, P, 1e-5, 8, P, P, NUL]
    for i in (0, 1, 2, 3, 6, 7):
        add('sisr_bn_eval_consts', BADARG, 'null_arg%d' % i, *(ok[:i] + [NUL] + ok[i + 1:]))
    add('sisr_bn_eval_consts', BADARG, 'C0', *(ok[:5] + [0] + ok[6:]))
    # sisr_eltwise_res_affine(x1, slope1_p, slope1, x2, pa, pd, y, P, C, dt, stream)
    ok = [P, NUL, 0.25, P, P, P, P, 10, 8, 0, NUL]
    for what, i, v in (('null_x1', 0, NUL), ('null_y', 6, NUL), ('P0', 7, 0), ('C0', 8, 0), ('C_and_3', 8, 6),
                       ('pa_without_pd', 5, NUL), ('pa_without_x2', 3, NUL)):
        add('sisr_eltwise_res_affine', BADARG, what, *(ok[:i] + [v] + ok[i + 1:]))
    # sisr_prelu_slope_grad(dy, pre, n, work, out, dt, stream): 16-byte loads of dy and pre
    ok = [P, P, 100, P, P, 0, NUL]
    for what, i, v in (('null_dy', 0, NUL), ('null_pre', 1, NUL), ('null_work', 3, NUL), ('null_out', 4, NUL), ('n0', 2, 0),
                       ('misaligned_dy', 0, Q), ('misaligned_pre', 1, Q), ('misaligned_pre_8', 1, P + 8)):
        add('sisr_prelu_slope_grad', BADARG, what, *(ok[:i] + [v] + ok[i + 1:]))
    # sisr_add(a, b, y, n, dt, stream): 16-byte accesses of all three; dt 0, 7 and 4 only
    ok = [P, P, P, 100, 0, NUL]
    for what, i, v in (('null_a', 0, NUL), ('null_b', 1, NUL), ('null_y', 2, NUL), ('n0', 3, 0), ('misaligned_a', 0, Q),
                       ('misaligned_b', 1, Q), ('misaligned_y', 2, P + 2)):
        add('sisr_add', BADARG, what, *(ok[:i] + [v] + ok[i + 1:]))
    for dt in (1, 2, 3, 5, 6):
        add('sisr_add', UNSUPPORTED, 'dt%d' % dt, *(ok[:4] + [dt, NUL]))
    return c


@pytest.mark.parametrize('fn,want,args', _cases())
def test_glue_entry_point_rejects_before_launch(lib, fn, want, args):
    assert getattr(lib, fn)(*args) == want
