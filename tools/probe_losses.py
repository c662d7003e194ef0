"""fused losses (losses.py, csrc/losses.hip) beside the torch glue they replace, forward + backward, in one process on the same
tensors: python tools/probe_losses.py [--reps 200] [--out profiles/losses_probe.json]

Content loss at n = 17,694,720 (B16 / HR 96^2 features of MaskedVGG(0b01111): cfg2 / cfg3) and n = 70,778,880 (HR 192^2: cfg4), the
gradient going to the fake side only, as in the G step; BCE at n = 16 with the label tensor, the loss weight and the mean(p)
statistic that surround it in train.py.  After a warm-up the two variants alternate, every repetition between its own pair of
device events; the median is reported (and the mean).  Measured twice: launched eagerly (host launch work included where the
device outruns it) and replayed from a HIP graph of the same calls (graph.GraphedStep: device time alone, the way bench.py runs
a step).  The fused kernels' bytes/s is the 5 passes they need (5 x 4n bytes) over the graphed time, kernel boundaries included.
Gate (content loss, both sizes, both ways of launching): fused time <= torch time / 1.5.  Refuses to run without a GPU."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

HBM_PEAK = 8.0e12           # bytes/s, MI355X specification
GATE = 1.5
CONTENT_SIZES = [17694720, 70778880]
BCE_N = 16


def alternate(variants, reps, warmup=20):
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


def summary(us):
    return dict(median_us=round(statistics.median(us), 2), mean_us=round(statistics.fmean(us), 2), min_us=round(min(us), 2))


def measure(fused, glue, reps):
    """eager and graphed timings of the two closures -> dict"""
    from gpu_helpers import pkg
    G = pkg('graph')
    out = {}
    for mode, variants in (('eager', dict(fused=fused, torch=glue)),
                           ('graph', dict(fused=G.GraphedStep(fused), torch=G.GraphedStep(glue)))):
        t = alternate(variants, reps)
        out[mode] = {k: summary(v) for k, v in t.items()}
        out[mode]['speedup'] = round(out[mode]['torch']['median_us'] / out[mode]['fused']['median_us'], 3)
    return out


def content_case(n, reps):
    from gpu_helpers import pkg
    Lo = pkg('losses')
    gen = torch.Generator(device='cuda').manual_seed(n % 1000)
    a = torch.randn(n, device='cuda', generator=gen)
    b = (a + 0.1 * torch.randn(n, device='cuda', generator=gen)).requires_grad_()

    def fused():
        b.grad = None
        loss = Lo.feature_mse(a, b)
        loss.backward()
        return loss.detach(), b.grad

    def glue():
        b.grad = None
        loss = torch.mean(torch.pow(a - b, 2))                 # train.py:186
        loss.backward()
        return loss.detach(), b.grad
    lf, gf = (t.clone() for t in fused())
    lg, gg = (t.clone() for t in glue())
    r = measure(fused, glue, reps)
    r['n'] = n
    r['loss_rel_diff'] = abs(float(lf) - float(lg)) / abs(float(lg))
    r['grad_max_rel_diff'] = float((gf - gg).abs().max() / gg.abs().max())
    bps = 5 * 4 * n / (r['graph']['fused']['median_us'] * 1e-6)
    r['fused_bytes_per_s'] = round(bps / 1e12, 3)              # TB/s over the graphed fused time
    r['fused_share_of_hbm_peak'] = round(bps / HBM_PEAK, 3)
    r['gate_1p5x'] = bool(r['eager']['speedup'] >= GATE and r['graph']['speedup'] >= GATE)
    return r


def bce_case(reps):
    from gpu_helpers import pkg
    Lo = pkg('losses')
    p = torch.rand(BCE_N, device='cuda', generator=torch.Generator(device='cuda').manual_seed(1)).requires_grad_()
    criterion, lw = torch.nn.BCELoss(), 5e-2

    def fused():
        p.grad = None
        loss, mean_p = Lo.bce_loss(p, 0.9, lw, return_mean=True)
        loss.backward()
        return loss.detach(), mean_p, p.grad

    def glue():
        p.grad = None
        label = torch.full((BCE_N,), 0.9, device='cuda')       # config.py:186-188
        loss = criterion(p, label) * lw                        # train.py:135, 73
        mean_p = p.detach().mean()                             # train.py:139 without the .item()
        loss.backward()
        return loss.detach(), mean_p, p.grad
    r = measure(fused, glue, reps)
    r['n'] = BCE_N
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'losses_probe.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('probe_losses: no GPU: nothing is measured without one')
    if args.reps < 200:
        print('probe_losses: fewer than 200 repetitions: a rehearsal, not a measurement')
    res = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, reps=args.reps, hbm_peak_bytes_per_s=HBM_PEAK,
               gate='fused forward + backward <= torch glue / %.1f (median of per-repetition device-event times)' % GATE,
               content=[content_case(n, args.reps) for n in CONTENT_SIZES], bce=bce_case(args.reps))
    res['gate_met'] = all(c['gate_1p5x'] for c in res['content'])
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))
    for c in res['content']:
        print('content n %9d: eager fused %8.1f us torch %8.1f us (%.2fx)   graph fused %8.1f us torch %8.1f us (%.2fx)   '
              'fused %.2f TB/s = %.0f %% of HBM peak' % (
                  c['n'], c['eager']['fused']['median_us'], c['eager']['torch']['median_us'], c['eager']['speedup'],
                  c['graph']['fused']['median_us'], c['graph']['torch']['median_us'], c['graph']['speedup'],
                  c['fused_bytes_per_s'], 100 * c['fused_share_of_hbm_peak']))
    b = res['bce']
    print('bce n %d: eager fused %.1f us torch %.1f us   graph fused %.1f us torch %.1f us'
          % (b['n'], b['eager']['fused']['median_us'], b['eager']['torch']['median_us'],
             b['graph']['fused']['median_us'], b['graph']['torch']['median_us']))
    print('gate %s' % ('met' if res['gate_met'] else 'NOT met'))


if __name__ == '__main__':
    main()
