"""The artifact-aware (LDL) loss (losses.artifact_loss, csrc/artifact.hip) beside the torch-op composition of the
same definition, in one process:  python tools/probe_artifact.py [--reps 200] [--out profiles/artifact_probe.json]

Shapes: (16, 3, 192, 192) -- the HR batch of the x2 training step -- and (16, 3, 96, 96), K = 7 (BasicSR's default).  Variants,
alternated after 10 warm-up rounds, every repetition between its own pair of device events, medians reported, as eager launches and
as graph replays (graph.GraphedStep):
  fused_fwd / fused_fwd_bwd   artifact_loss, and its backward pass through autograd (gradients of sr and gt);
  torch_fwd / torch_fwd_bwd   BasicSR's text: get_refined_artifact_map (reflect F.pad + two unfolds + torch.var + masked assignment)
                              under no_grad, then L1Loss(m * sr, m * gt), and its backward pass.
The forward moves at least three images and one map (24 MB at 192^2); the achieved rate over that count is reported beside the
times.  Times are reported, not asserted.  Refuses to run without a GPU."""
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

SHAPES, K = ((16, 3, 192, 192), (16, 3, 96, 96)), 7


def refined_artifact_map(img_gt, img_output, img_ema, ksize):
    residual_ema = torch.sum(torch.abs(img_gt - img_ema), 1, keepdim=True)
    residual_sr = torch.sum(torch.abs(img_gt - img_output), 1, keepdim=True)
    patch_level_weight = torch.var(residual_sr.clone(), dim=(-1, -2, -3), keepdim=True) ** (1 / 5)
    pad = (ksize - 1) // 2
    residual_pad = F.pad(residual_sr.clone(), pad=[pad, pad, pad, pad], mode='reflect')
    unfolded = residual_pad.unfold(2, ksize, 1).unfold(3, ksize, 1)
    pixel_level_weight = torch.var(unfolded, dim=(-1, -2), unbiased=True, keepdim=True).squeeze(-1).squeeze(-1)
    overall_weight = patch_level_weight * pixel_level_weight
    overall_weight[residual_sr < residual_ema] = 0
    return overall_weight


def variants_for(shape, Lm):
    gen = torch.Generator(device='cuda').manual_seed(1)
    gt = 2 * torch.rand(shape, device='cuda', generator=gen) - 1
    sr = (gt + 0.1 * torch.randn(shape, device='cuda', generator=gen)).requires_grad_(True)
    gt.requires_grad_(True)
    ema = (sr + 0.05 * torch.randn(shape, device='cuda', generator=gen)).detach()

    def fused(a, b):
        return Lm.artifact_loss(a, b, ema, K)

    def composed(a, b):
        with torch.no_grad():
            m = refined_artifact_map(b, a, ema, K)
        return F.l1_loss(m * a, m * b)

    def nograd(fn):
        def run():
            with torch.no_grad():
                return fn(sr.detach(), gt.detach())
        return run

    def bwd(fn):
        def run():
            sr.grad = gt.grad = None
            fn(sr, gt).backward()
            return sr.grad, gt.grad
        return run
    return dict(fused_fwd=nograd(fused), torch_fwd=nograd(composed), fused_fwd_bwd=bwd(fused), torch_fwd_bwd=bwd(composed))


def ratios(m):
    """fused / composition for every pair that was timed"""
    for op in ('fwd', 'fwd_bwd'):
        if 'fused_' + op in m and 'torch_' + op in m:
            m['fused_%s_over_torch_%s' % (op, op)] = round(m['fused_' + op] / m['torch_' + op], 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'artifact_probe.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('probe_artifact: no GPU: nothing is measured without one')
    if args.reps < 200:
        print('probe_artifact: fewer than 200 repetitions: a rehearsal, not a measurement')
    from gpu_helpers import pkg
    Lm, G = pkg('losses'), pkg('graph')
    res = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, reps=args.reps, ksize=K,
               timing='medians of per-repetition device-event times in microseconds, variants alternated after 10 warm-up rounds; eager '
                      'launches on one stream, then the same callables as graph.GraphedStep replays',
               composition='get_refined_artifact_map as BasicSR writes it (reflect F.pad + two unfolds + torch.var + masked assignment) '
                           'under no_grad, then F.l1_loss(m * sr, m * gt)',
               min_forward_bytes='three images read and one map written, 4 bytes each; the rate is that count over the fused forward time',
               shapes={})
    for shape in SHAPES:
        variants = variants_for(shape, Lm)
        n, c, h, w = shape
        entry = dict(min_forward_bytes=4 * n * h * w * (3 * c + 1))
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
            if 'fused_fwd' in entry[mode]:
                entry[mode]['fused_fwd_min_bytes_GBps'] = round(entry['min_forward_bytes'] / entry[mode]['fused_fwd'] * 1e-3, 1)
        res['shapes']['x'.join(str(v) for v in shape)] = entry
        print(json.dumps({str(shape): entry}), flush=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
