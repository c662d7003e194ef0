"""fused JPEG round trip (jpeg.py, csrc/jpeg.hip) beside the torch-op composition of the same definition, in one process:
  python tools/probe_jpeg.py [--reps 200] [--out profiles/jpeg_probe.json]

Shapes: (16, 3, 96, 96) -- the LR batch of the x2 training step -- and (16, 3, 192, 192); 4:2:0, a quality per sample in 30 .. 95,
clamp on.  Variants, alternated after 10 warm-up rounds, every repetition between its own pair of device events, medians reported:
  fused_fwd                       sisr_jpeg_fwd with the tables given (one launch);
  torch_fwd_a/_b                  the composition: colour matmul, replicate pad, avg_pool2d, F.unfold, two matmuls with the DCT matrix,
                                  divide, round, multiply, two matmuls back, F.fold, repeat_interleave, colour matmul, clamp -- measured
                                  TWICE in the same alternation: the difference of its two medians is the run-to-run spread of this run;
  fused_fwd_bwd_ste / _cubic      forward and the backward pass through autograd, gradient in the image.
The two forwards are also compared at each shape (share of elements that agree to 1e-4: a coefficient at a rounding tie may decode
differently).  No ratio is fixed in advance: the numbers are a fact for DESIGN.md section 20.  Per-kernel times come from a
separate run under rocprofv3 --kernel-trace --stats.  Refuses to run without a GPU."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from probe_degrade import alternate  # noqa: E402

SHAPES = [(16, 3, 96, 96), (16, 3, 192, 192)]
COLOUR = [[0.299, 0.587, 0.114], [-0.168735892, -0.331264108, 0.5], [0.5, -0.418687589, -0.081312411]]


def torch_composition(tables):
    """the definition in fp32 torch ops for 4:2:0 and MCU-multiple sizes -> fn(x)"""
    dev = tables.device
    M = torch.tensor(COLOUR, device=dev)
    Minv = torch.linalg.inv(M.double()).float()
    k = torch.arange(8, device=dev, dtype=torch.float64)
    D = torch.cos((2 * k[None, :] + 1) * k[:, None] * math.pi / 16) * 0.5
    D[0] = math.sqrt(1 / 8)
    D = D.float()

    def plane(q, t):                                        # q [N, 1, h, w], t [N, 8, 8]
        n, _, h, w = q.shape
        b = F.unfold(q, 8, stride=8).transpose(1, 2).reshape(n, -1, 8, 8)
        c = D @ b @ D.T
        tt = t[:, None]
        chat = torch.round(c / tt) * tt
        r = (D.T @ chat @ D).reshape(n, -1, 64).transpose(1, 2)
        return F.fold(r, (h, w), 8, stride=8)

    def run(x):
        p = (x + 1) * 127.5
        ycc = torch.einsum('ij,njhw->nihw', M, p)
        y, cbcr = ycc[:, :1] - 128, F.avg_pool2d(ycc[:, 1:], 2)
        y = plane(y, tables[:, 0]) + 128
        cb, cr = plane(cbcr[:, :1], tables[:, 1]), plane(cbcr[:, 1:], tables[:, 1])
        up = torch.cat([cb, cr], dim=1).repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
        rgb = torch.einsum('ij,njhw->nihw', Minv, torch.cat([y, up], dim=1))
        return rgb.clamp(0, 255) / 127.5 - 1

    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'jpeg_probe.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('probe_jpeg: no GPU: nothing is measured without one')
    if args.reps < 200:
        print('probe_jpeg: fewer than 200 repetitions: a rehearsal, not a measurement')
    from gpu_helpers import pkg
    J = pkg('jpeg')
    res = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, reps=args.reps, subsampling='420', quality='30..95 per sample',
               timing='medians of per-repetition device-event times, eager launches on one stream, variants alternated after 10 warm-up rounds',
               shapes={})
    for shape in SHAPES:
        gen = torch.Generator(device='cuda').manual_seed(1)
        x = (2 * torch.rand(shape, device='cuda', generator=gen) - 1).requires_grad_(True)
        dy = torch.randn(shape, device='cuda', generator=gen)
        q = J.expected_quality(1, 0, shape[0], 30, 95)
        tables = torch.from_numpy(np.stack([np.stack(J.quant_tables(int(v))) for v in q])).float().cuda()
        composed = torch_composition(tables)

        def fused(inp=x, grad='ste'):
            return J.jpeg_roundtrip(inp, tables, '420', grad, True)

        def bwd(grad):
            def run():
                x.grad = None
                fused(x, grad).backward(dy)
            return run

        with torch.no_grad():
            a, b = fused(x.detach()), composed(x.detach())
            agree = float(((a - b).abs() <= 1e-4).float().mean())
            variants = dict(torch_fwd_a=lambda: composed(x.detach()), fused_fwd=lambda: fused(x.detach()),
                            torch_fwd_b=lambda: composed(x.detach()))
            t = {key: statistics.median(v) for key, v in alternate(variants, args.reps).items()}
        t.update({key: statistics.median(v) for key, v in
                  alternate(dict(fused_fwd_bwd_ste=bwd('ste'), fused_fwd_bwd_cubic=bwd('cubic')), args.reps).items()})
        nbytes = 8 * x.numel()
        res['shapes']['x'.join(map(str, shape))] = dict(
            median_us={key: round(v, 2) for key, v in t.items()},
            torch_fwd_spread_us=round(abs(t['torch_fwd_a'] - t['torch_fwd_b']), 2),
            fused_over_torch_fwd=round(t['fused_fwd'] / (0.5 * (t['torch_fwd_a'] + t['torch_fwd_b'])), 4),
            bytes_moved_by_the_forward=nbytes, fused_fwd_gb_per_s=round(nbytes / t['fused_fwd'] * 1e-3, 1),
            share_of_elements_where_the_two_forwards_agree_to_1e_4=agree)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
