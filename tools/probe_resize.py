"""The device resize (resize.py, csrc/resize.hip) beside torch's own operator, in one process:
python tools/probe_resize.py [--reps 200] [--out profiles/resize_probe.json]

Cases: (16, 3, 192, 192) -> (136, 136), (16, 3, 192, 192) -> (96, 96), (16, 3, 96, 96) -> (192, 192).  Variants, alternated after 10
warm-up rounds, every repetition between its own pair of device events, medians reported, as eager launches and as graph replays
(graph.GraphedStep):
  (a) <mode>_fwd / <mode>_fwd_bwd       resize with one mode for the batch, against torch_<mode>_*: F.interpolate on the device;
  (b) mixed_fwd / mixed_fwd_bwd         resize with a per-sample device table, against torch_mixed_*: the composition that gives
                                        per-sample modes capturably -- three F.interpolate calls and a torch.where over the batch;
  (c) degrader_*                        HighOrderDegrader (192 -> 136 -> 96) with resize_probs=(1/3, 1/3, 1/3) against
                                        resize_probs=None, forward and forward + backward.
Times are reported, not asserted.  Refuses to run without a GPU."""
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

CASES = (((16, 3, 192, 192), (136, 136)), ((16, 3, 192, 192), (96, 96)), ((16, 3, 96, 96), (192, 192)))
MODES = ('area', 'bilinear', 'bicubic')


def interp(x, size, mode):
    return F.interpolate(x, size=size, mode=mode) if mode == 'area' else F.interpolate(x, size=size, mode=mode, align_corners=False)


def variants_for(shape, size, R):
    n = shape[0]
    gen = torch.Generator(device='cuda').manual_seed(1)
    x = (2 * torch.rand(shape, device='cuda', generator=gen) - 1).requires_grad_(True)
    dy = torch.randn(shape[:2] + size, device='cuda', generator=gen)
    table = (torch.arange(n, device='cuda') % 3).to(torch.int32)
    sel = [(table == m).view(n, 1, 1, 1) for m in range(3)]

    def torch_mixed(inp):
        a, b, c = (interp(inp, size, m) for m in MODES)
        return torch.where(sel[0], a, torch.where(sel[1], b, c))

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
    v = {}
    for m in MODES:
        ours, theirs = (lambda inp, m=m: R.resize(inp, size, m)), (lambda inp, m=m: interp(inp, size, m))
        v[m + '_fwd'], v['torch_' + m + '_fwd'] = nograd(ours), nograd(theirs)
        v[m + '_fwd_bwd'], v['torch_' + m + '_fwd_bwd'] = bwd(ours), bwd(theirs)
    mixed = lambda inp: R.resize(inp, size, table)      # noqa: E731
    v['mixed_fwd'], v['torch_mixed_fwd'] = nograd(mixed), nograd(torch_mixed)
    v['mixed_fwd_bwd'], v['torch_mixed_fwd_bwd'] = bwd(mixed), bwd(torch_mixed)
    return v


def degrader_variants(D):
    shape = (16, 3, 192, 192)
    gen = torch.Generator(device='cuda').manual_seed(2)
    x = (2 * torch.rand(shape, device='cuda', generator=gen) - 1).requires_grad_(True)
    dy = torch.randn((16, 3, 96, 96), device='cuda', generator=gen)
    v = {}
    for name, probs in (('degrader_plain', None), ('degrader_resize', (1 / 3, 1 / 3, 1 / 3))):
        d = D.HighOrderDegrader(mid_size=(136, 136), seed=1, resize_probs=probs)

        def fwd(d=d):
            with torch.no_grad():
                return d(x.detach(), (96, 96))

        def fwd_bwd(d=d):
            x.grad = None
            d(x, (96, 96)).backward(dy)
            return x.grad
        v[name + '_fwd'], v[name + '_fwd_bwd'] = fwd, fwd_bwd
    return v


def ratios(m):
    """ours / torch (and the degrader with drawn resamplers / without) for every pair that was timed"""
    pairs = [('%s_%s_over_torch' % (k, op), '%s_%s' % (k, op), 'torch_%s_%s' % (k, op)) for k in MODES + ('mixed',) for op in ('fwd', 'fwd_bwd')]
    pairs += [('degrader_resize_%s_over_plain' % op, 'degrader_resize_' + op, 'degrader_plain_' + op) for op in ('fwd', 'fwd_bwd')]
    for name, ours, theirs in pairs:
        if ours in m and theirs in m:
            m[name] = round(m[ours] / m[theirs], 4)


def measure(variants, reps, G):
    entry = {}
    t = alternate(variants, reps)
    entry['eager_median_us'] = {k: round(statistics.median(v), 2) for k, v in t.items()}
    graphed, failed = {}, {}
    for k, fn in variants.items():
        try:
            graphed[k] = G.GraphedStep(fn)
        except G.GraphCaptureError as e:
            failed[k] = str(e)
    t = alternate(graphed, reps)
    entry['graph_median_us'] = {k: round(statistics.median(v), 2) for k, v in t.items()}
    if failed:
        entry['graph_capture_failed'] = failed
    for mode in ('eager_median_us', 'graph_median_us'):
        ratios(entry[mode])
    return entry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'resize_probe.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('probe_resize: no GPU: nothing is measured without one')
    if args.reps < 200:
        print('probe_resize: fewer than 200 repetitions: a rehearsal, not a measurement')
    from gpu_helpers import pkg
    R, D, G = pkg('resize'), pkg('degrade'), pkg('graph')
    res = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, reps=args.reps,
               timing='medians of per-repetition device-event times in microseconds, variants alternated after 10 warm-up rounds; eager '
                      'launches on one stream, then the same callables as graph.GraphedStep replays',
               compositions='torch_<mode>: F.interpolate on the device (align_corners=False; area as it is); torch_mixed: three '
                            'F.interpolate calls and a torch.where over the batch; degrader_plain: HighOrderDegrader(resize_probs=None), '
                            'degrader_resize: resize_probs=(1/3, 1/3, 1/3), both 192 -> 136 -> 96 with the two published stages',
               cases={})
    for shape, size in CASES:
        key = '%s->%s' % ('x'.join(str(v) for v in shape), 'x'.join(str(v) for v in size))
        res['cases'][key] = entry = measure(variants_for(shape, size, R), args.reps, G)
        print(json.dumps({key: entry}), flush=True)
    res['degrader'] = entry = measure(degrader_variants(D), args.reps, G)
    print(json.dumps({'degrader': entry}), flush=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
