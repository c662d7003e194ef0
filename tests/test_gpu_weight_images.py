"""GPU: every packed weight image engine.prepare_weights hands to a conv kernel, bit for bit against the layouts include/sisr_hip.h
documents -- the forward image, the stride-1 data gradient or the four parity classes of a stride-2 one, in the fp32 order (with
the LDS-order copy), the bf16 order (with the lane-order copy) and the conv_deep.hip row format.

tests/weights_cases.py builds the reference on the CPU: ONE gather under one tap map (image_values) and one function per storage
order.  fp32 and bf16 images hold fl32(W_orig * fl32(1 / sigma)) -- sigma read back from the device, one IEEE product --, bf16
by round to nearest even; conv_deep.hip images hold W_orig itself.  The whole image is compared, every padding slot included."""
import numpy as np
import pytest
import torch

import weights_cases as WC
from gpu_helpers import FakeConv, pkg

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('build', ['fp32', 'bf16x3', 'bf16'])
def test_packed_images_bit_for_bit(build):
    E = pkg('engine')
    before = E.PRECISION
    E.set_precision(build)
    try:
        refs, items = [], []
        for i, (cin, cout, k, stride, shuffle2, h, w) in enumerate(WC.IMAGE_CASES[build]):
            gm = E.ConvGeom(cin, cout, k, stride, shuffle2=bool(shuffle2))
            wm, u, v = WC.sn_inputs((cout, cin, k), seed=60 + i)
            refs.append(FakeConv(wm.reshape(cout, cin, k, k).contiguous().cuda(), None, gm, u.cuda(), v.cuda()))
            items.append((refs[-1], 2, h, w))
        preps, keep = E.prepare_weights(items, training=False)
        torch.cuda.synchronize()
        n_images = n_slots = 0
        for i, p in enumerate(preps):
            WC.check_reach(E, build, i, p)
            gm = p.ref.geom
            sigma = np.float32(p.sigma.cpu().item())
            assert sigma != np.float32(1), 'spectral norm is on: 1 / sigma must not be 1'
            inv = torch.tensor(np.float32(1) / sigma)
            assert p.inv_sigma.cpu().view(torch.int32).item() == inv.view(torch.int32).item()
            w4 = p.ref.weight.cpu()
            views = [p.wpk_fwd] + (list(p.wpk_dgrad) if isinstance(p.wpk_dgrad, (list, tuple)) else [p.wpk_dgrad])
            specs = [s for s in WC.image_specs(E, p)]
            assert specs[0] is not None and sum(s is not None for s in specs) in (2, 5)
            for spec, view in zip(specs, views):
                if spec is None:
                    continue
                want, _ = WC.expected_image(spec, w4, None if spec.fmt == WC.IMG_DEEP else inv, gm.shuffle2)
                assert want.numel() == spec.old_slots and view.numel() >= want.numel(), (build, i, spec.name)
                got = view[:want.numel()].cpu().view(torch.int32)
                bad = int((got != want).sum())
                print('%s %d>%d k%d s%d %s: %d slots, %d differ' % (build, gm.cin, gm.cout, gm.k, gm.stride, spec.name, want.numel(), bad))
                assert bad == 0, (build, i, spec.name, bad)
                n_images += 1
                n_slots += want.numel()
        print('%s: %d images, %d slots compared' % (build, n_images, n_slots))
    finally:
        E.set_precision(before)
