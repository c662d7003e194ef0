"""fused blur + resample + noise degradation (degrade.py, csrc/degrade.hip) beside the torch-op composition of the same operator, in
one process:  python tools/probe_degrade.py [--reps 200] [--out profiles/degrade_probe.json]

Shape: (16, 3, 192, 192) -> (96, 96), K = 21, noise on -- the x2 training batch.  Variants, alternated after a warm-up, every
repetition between its own pair of device events, medians reported:
  fused_fwd        sisr_degrade_fwd with the kernels given (one launch);
  fused_draw_fwd   Degrader.__call__: sisr_degrade_draw + sisr_degrade_fwd (two launches, what a training step calls);
  torch_fwd_a/_b   F.pad(replicate), a grouped F.conv2d with per-sample weights, the package's bicubic kernel (no clamp), randn * sigma,
                   add, clamp -- what the code before this operator offers; measured TWICE in the same alternation: the difference of
                   its two medians is the run-to-run spread of this run;
  fused_fwd_bwd / torch_fwd_bwd   forward and the backward pass through autograd, gradient in the image alone.
The two forwards are also compared (noise off) at this size.  No ratio is fixed in advance: the numbers are a fact for DESIGN.md
section 18.  Per-kernel times come from a separate run under rocprofv3 --kernel-trace --stats.  Refuses to run without a GPU."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

SHAPE, SIZE, KSIZE = (16, 3, 192, 192), (96, 96), 21


def alternate(variants, reps, warmup=10):
    """variants: {name: fn}; -> {name: [microseconds per repetition]}"""
    for _ in range(warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    events = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            events[k].append((e0, e1))
    torch.cuda.synchronize()
    return {k: [e0.elapsed_time(e1) * 1e3 for e0, e1 in v] for k, v in events.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'degrade_probe.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('probe_degrade: no GPU: nothing is measured without one')
    if args.reps < 200:
        print('probe_degrade: fewer than 200 repetitions: a rehearsal, not a measurement')
    from gpu_helpers import pkg
    D, U = pkg('degrade'), pkg('utils')
    n, c, h, w = SHAPE
    R = (KSIZE - 1) // 2
    gen = torch.Generator(device='cuda').manual_seed(1)
    x = (2 * torch.rand(SHAPE, device='cuda', generator=gen) - 1).requires_grad_(True)
    dy = torch.randn((n, c) + SIZE, device='cuda', generator=gen)
    d = D.Degrader(ksize=KSIZE, sigma=(0.2, 3.0), noise=(0.01, 0.1), seed=1)
    k, sigma, step = d.draw(n)
    wgt = k.repeat_interleave(c, dim=0)[:, None]

    def torch_linear(inp):
        xp = F.pad(inp, (R, R, R, R), mode='replicate').reshape(1, n * c, h + 2 * R, w + 2 * R)
        return U._subsampling_interpolation(F.conv2d(xp, wgt, groups=n * c).reshape(n, c, h, w), SIZE)

    def torch_fwd(inp=x):
        r = torch_linear(inp)
        return (r + sigma[:, None, None, None] * torch.randn_like(r)).clamp(-1, 1)

    def fused_fwd(inp=x):
        return D.degrade(inp, SIZE, k, sigma, step, d.seed, d.rank)

    def bwd(fwd):
        def run():
            x.grad = None
            fwd().backward(dy)
        return run

    with torch.no_grad():
        a, b = D.degrade(x, SIZE, k, clamp=False), torch_linear(x)
    agreement = float((a - b).abs().max())
    with torch.no_grad():
        variants = dict(torch_fwd_a=lambda: torch_fwd(x.detach()), fused_fwd=lambda: fused_fwd(x.detach()),
                        torch_fwd_b=lambda: torch_fwd(x.detach()), fused_draw_fwd=lambda: d(x.detach(), SIZE))
        t = {key: statistics.median(v) for key, v in alternate(variants, args.reps).items()}
    t.update({key: statistics.median(v) for key, v in alternate(dict(torch_fwd_bwd=bwd(torch_fwd), fused_fwd_bwd=bwd(fused_fwd)),
                                                                args.reps).items()})
    macs = n * c * h * w * KSIZE * KSIZE
    res = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, reps=args.reps, shape=SHAPE, size=SIZE, ksize=KSIZE,
               timing='medians of per-repetition device-event times, eager launches on one stream, variants alternated after 10 warm-up rounds',
               median_us={key: round(v, 2) for key, v in t.items()},
               torch_fwd_spread_us=round(abs(t['torch_fwd_a'] - t['torch_fwd_b']), 2),
               fused_over_torch_fwd=round(t['fused_fwd'] / (0.5 * (t['torch_fwd_a'] + t['torch_fwd_b'])), 4),
               fused_over_torch_fwd_bwd=round(t['fused_fwd_bwd'] / t['torch_fwd_bwd'], 4),
               blur_macs_of_the_operator=macs, fused_fwd_blur_gmacs_per_s=round(macs / t['fused_fwd'] * 1e-3, 1),
               max_abs_difference_of_the_two_forwards_without_noise=agreement)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
