"""Gaussian filter and unsharp mask (filters.py, csrc/gauss.hip) beside two torch-op compositions of the same
definition, in one process:  python tools/probe_usm.py [--reps 200] [--out profiles/usm_probe.json]

Shapes: (16, 3, 192, 192) -- the HR batch of the x2 training step -- and (16, 3, 96, 96), K = 51 (sigma 8: Real-ESRGAN's USM).
Variants, alternated after 10 warm-up rounds, every repetition between its own pair of device events, medians reported, as eager
launches and as graph replays (graph.GraphedStep):
  blur_fwd / blur_fwd_bwd / usm   gaussian_blur, its backward pass through autograd, usm_sharpen;
  (a) torch_full_*                Real-ESRGAN's form: reflect F.pad + ONE grouped K x K F.conv2d (its filter2D);
  (b) torch_sep_*                 the separable form: reflect F.pad + two grouped 1-D F.conv2d.
The USM compositions are USMSharp.forward written with either blur.  Times are reported, not asserted.  Refuses to run without a
GPU."""
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

from probe_degrade import alternate  # noqa: E402

SHAPES, K = ((16, 3, 192, 192), (16, 3, 96, 96)), 51


def variants_for(shape, Fm):
    n, c, h, w = shape
    R = K // 2
    gen = torch.Generator(device='cuda').manual_seed(1)
    x = (2 * torch.rand(shape, device='cuda', generator=gen) - 1).requires_grad_(True)
    dy = torch.randn(shape, device='cuda', generator=gen)
    t = torch.from_numpy(Fm.gaussian_taps(K)).cuda()
    k2 = torch.outer(t, t).view(1, 1, K, K).repeat(n * c, 1, 1, 1).contiguous()
    kh, kv = t.view(1, 1, 1, K).repeat(n * c, 1, 1, 1).contiguous(), t.view(1, 1, K, 1).repeat(n * c, 1, 1, 1).contiguous()

    def pad(inp):
        return F.pad(inp, (R, R, R, R), mode='reflect').reshape(1, n * c, h + 2 * R, w + 2 * R)

    def full(inp):
        return F.conv2d(pad(inp), k2, groups=n * c).reshape(shape)

    def sep(inp):
        return F.conv2d(F.conv2d(pad(inp), kh, groups=n * c), kv, groups=n * c).reshape(shape)

    def fused(inp):
        return Fm.gaussian_blur(inp, K)

    def usm_of(blur):
        def run(img, weight=0.5, threshold=10.0):
            b = blur(img)
            residual = img - b
            mask = (residual.abs() * 127.5 > threshold).float()
            soft = blur(mask)
            sharp = (img + weight * residual).clamp(-1, 1)
            return soft * sharp + (1 - soft) * img
        return run

    def nograd(fn):
        def run():
            with torch.no_grad():
                return fn(x.detach())
        return run

    def bwd(fn):
        def run():
            x.grad = None
            fn(x).backward(dy)
            return x.grad
        return run
    return dict(blur_fwd=nograd(fused), torch_full_fwd=nograd(full), torch_sep_fwd=nograd(sep),
                blur_fwd_bwd=bwd(fused), torch_full_fwd_bwd=bwd(full), torch_sep_fwd_bwd=bwd(sep),
                usm=lambda: Fm.usm_sharpen(x), torch_full_usm=nograd(usm_of(full)), torch_sep_usm=nograd(usm_of(sep)))


def ratios(m):
    """fused / composition for every pair that was timed"""
    pairs = [('blur_%s_over_torch_%s' % (op, ref), 'blur_' + op, 'torch_%s_%s' % (ref, op)) for op in ('fwd', 'fwd_bwd') for ref in ('full', 'sep')]
    pairs += [('usm_over_torch_%s' % ref, 'usm', 'torch_%s_usm' % ref) for ref in ('full', 'sep')]
    for name, ours, theirs in pairs:
        if ours in m and theirs in m:
            m[name] = round(m[ours] / m[theirs], 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'usm_probe.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('probe_usm: no GPU: nothing is measured without one')
    if args.reps < 200:
        print('probe_usm: fewer than 200 repetitions: a rehearsal, not a measurement')
    from gpu_helpers import pkg
    Fm, G = pkg('filters'), pkg('graph')
    res = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, reps=args.reps, ksize=K, sigma=8.0,
               timing='medians of per-repetition device-event times in microseconds, variants alternated after 10 warm-up rounds; eager '
                      'launches on one stream, then the same callables as graph.GraphedStep replays',
               compositions='torch_full: reflect F.pad + one grouped K x K conv2d (Real-ESRGAN filter2D); torch_sep: reflect F.pad + two '
                            'grouped 1-D conv2d', shapes={})
    for shape in SHAPES:
        variants = variants_for(shape, Fm)
        entry = {}
        t = alternate(variants, args.reps)
        entry['eager_median_us'] = {k: round(statistics.median(v), 2) for k, v in t.items()}
        graphed, failed = {}, {}
        for k, fn in variants.items():
            try:
                graphed[k] = G.GraphedStep(fn)
            except G.GraphCaptureError as e:
                failed[k] = str(e)
        t = alternate(graphed, args.reps)
        entry['graph_median_us'] = {k: round(statistics.median(v), 2) for k, v in t.items()}
        if failed:
            entry['graph_capture_failed'] = failed
        for mode in ('eager_median_us', 'graph_median_us'):
            ratios(entry[mode])
        res['shapes']['x'.join(str(v) for v in shape)] = entry
        print(json.dumps({str(shape): entry}), flush=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
