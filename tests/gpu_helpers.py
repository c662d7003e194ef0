"""Helpers for the -m gpu parity tests: they drive the product through its public surfaces (the
nn.Module drop-ins and the engine wrappers over the C ABI) and compare with the CPU oracle."""
import importlib

import torch

PKG = 'single-image-super-resolution_amd'


def pkg(sub=None):
    return importlib.import_module(PKG + ('.' + sub if sub else ''))


class FakeConv:
    """minimal ConvRef stand-in for kernel-level tests"""

    def __init__(self, weight, bias, geom, u=None, v=None):
        self.weight, self.bias, self.geom, self.u, self.v = weight, bias, geom, u, v


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def maxrel(a, b):
    a = a.detach().double().cpu().reshape(-1)
    b = b.detach().double().cpu().reshape(-1)
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))


# ---- kernel-level value tests through the C ABI (test_gpu_glue.py, test_gpu_weights.py) -------------------------------------------
SENT = -1536.0                      # exact in fp32 and bf16, never produced by the seeded inputs
GUARD = 64                          # elements on each side (keeps the body 128-byte aligned in both formats)
F32, BF16 = torch.float32, torch.bfloat16


def _bits(t):
    return t.view(torch.int32 if t.dtype == F32 else torch.int16)


class Buf:
    """an output of `numel` elements between two sentinel guards; `fill`: what the body holds before every launch"""

    def __init__(self, numel, dtype=F32, fill=SENT):
        self.numel, self.fill = numel, fill
        self.whole = torch.empty(numel + 2 * GUARD, dtype=dtype, device='cuda')
        self.body = self.whole[GUARD:GUARD + numel]
        self.reset()

    def reset(self):
        self.whole.fill_(SENT)
        if self.fill != SENT:
            self.body.fill_(self.fill)

    def ptr(self, offset=0):
        return self.body.data_ptr() + offset * self.body.element_size()

    def guards_intact(self):
        lo, hi = self.whole[:GUARD], self.whole[GUARD + self.numel:]
        return bool((lo == SENT).all()) and bool((hi == SENT).all())

    def cpu(self):
        return self.body.cpu()


def run2(call, outs):
    """launch twice from the same pre-fill: status 0, guards intact, identical bits; leaves the second run's results in place"""
    first = None
    for rep in range(2):
        for o in outs:
            o.reset()
        status = call()
        torch.cuda.synchronize()
        assert status == 0, status
        for k, o in enumerate(outs):
            assert o.guards_intact(), 'guard of output %d changed' % k
        if rep == 0:
            first = [o.body.clone() for o in outs]
    for a, o in zip(first, outs):
        assert torch.equal(_bits(a), _bits(o.body)), 'two runs differ'


def assert_within(got, ref64, bound, what=''):
    """element by element; prints the worst ratio before asserting"""
    err = (got.double() - ref64).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    worst = float(err.max()) if err.numel() else 0.0
    print('%s: max err %.3e, max err/bound %.3f' % (what, worst, ratio))
    assert bool((err <= bound).all()), (what, worst, ratio)
