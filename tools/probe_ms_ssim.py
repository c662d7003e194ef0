"""fused multi-scale SSIM loss (losses.ms_ssim_loss, csrc/ms_ssim.hip) beside the torch-op composition of the same definition, in one
process on the same tensors: python tools/probe_ms_ssim.py [--reps 200] [--out profiles/ms_ssim_probe.json]

Cases: 16 x 3 x 192 x 192 with the five default scales (bench.py's HR patches) and 16 x 3 x 96 x 96 with the first three weights
(the HR patches of the other configs), the gradient going to the fake side only, as in the G step.  The composition is the
definition written with torch ops (per scale ten single-channel F.conv2d windows, the cs / l maps
elementwise, F.avg_pool2d between the scales, torch.where for the t <= 0 rule, autograd backward).  Timed: the forward alone (under
no_grad) and forward + backward.  After a warm-up the two variants alternate, every repetition between its own pair of device events;
the median is reported (and the mean).  Measured twice: launched eagerly (host launch work included where the device outruns it)
and replayed from a HIP graph of the same calls (graph.GraphedStep: device time alone).  If the composition cannot be captured, that
is recorded and the graphed comparison is left out.  These times are facts to record, not a condition.  Refuses to run without a
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

WINDOW, DATA_RANGE = 11, 2.0
CASES = [((16, 3, 192, 192), 5), ((16, 3, 96, 96), 3)]


def composition(a, b, window, wts):
    """the definition with torch ops; window [11] and wts [M, 1, 1] are device tensors (nothing is copied from the host, so the
    calls can be captured) -> 0-dim loss (mean over the batch)"""
    c1, c2 = (0.01 * DATA_RANGE) ** 2, (0.03 * DATA_RANGE) ** 2
    m, terms = wts.shape[0], []
    for j in range(m):
        n, c, h, w = a.shape

        def win(t):
            t = t.reshape(n * c, 1, h, w)
            return F.conv2d(F.conv2d(t, window.view(1, 1, WINDOW, 1)), window.view(1, 1, 1, WINDOW))
        mu_a, mu_b = win(a), win(b)
        var_a, var_b, cov = win(a * a) - mu_a ** 2, win(b * b) - mu_b ** 2, win(a * b) - mu_a * mu_b
        cs = (2 * cov + c2) / (var_a + var_b + c2)
        if j == m - 1:
            cs = cs * (2 * mu_a * mu_b + c1) / (mu_a ** 2 + mu_b ** 2 + c1)
        terms.append(cs.reshape(n, c, -1).mean(dim=2))
        if j < m - 1:
            a, b = F.avg_pool2d(a, 2), F.avg_pool2d(b, 2)
    terms = torch.stack(terms)
    positive = (terms > 0).all(dim=0)
    powers = torch.where(positive.unsqueeze(0), terms, torch.ones_like(terms)) ** wts
    score = torch.where(positive, powers.prod(dim=0), torch.zeros_like(powers[0]))
    return (1 - score.mean(dim=1)).mean()


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


def batch(shape):
    """(a, b): a requires a gradient (the fake side)"""
    gen = torch.Generator(device='cuda').manual_seed(shape[-1])
    b = torch.rand(shape, device='cuda', generator=gen) * 2 - 1
    a = (b + 0.1 * torch.randn(shape, device='cuda', generator=gen)).clamp(-1, 1).requires_grad_()
    return a, b


def measure(G, fused, glue, reps):
    """-> {'eager': ..., 'graph': ...} for one pair of variants"""
    r = {}
    t = alternate(dict(fused=fused, torch=glue), reps)
    r['eager'] = {k: summary(v) for k, v in t.items()}
    variants, r['graph'] = {}, {}
    for name, fn in (('fused', fused), ('torch', glue)):          # each capture on its own: a variant that cannot be captured is named
        try:
            variants[name] = G.GraphedStep(fn)
        except G.GraphCaptureError as e:
            r['graph'][name + '_error'] = str(e)
    r['graph'].update({k: summary(v) for k, v in alternate(variants, reps).items()})
    for mode in ('eager', 'graph'):
        if 'fused' in r[mode] and 'torch' in r[mode]:
            r[mode]['torch_over_fused'] = round(r[mode]['torch']['median_us'] / r[mode]['fused']['median_us'], 3)
    return r


def case(shape, scales, reps):
    from gpu_helpers import pkg
    Lo, G = pkg('losses'), pkg('graph')
    weights = pkg('metrics').MS_SSIM_WEIGHTS[:scales]
    a, b = batch(shape)
    window = torch.exp(-(torch.arange(WINDOW, dtype=torch.float64) - WINDOW // 2) ** 2 / (2 * 1.5 ** 2))
    window = (window / window.sum()).float().cuda()
    wts = torch.tensor(weights, dtype=torch.float32).view(scales, 1, 1).cuda()

    def fused_fwd():
        with torch.no_grad():
            return Lo.ms_ssim_loss(a, b, weights=weights)

    def glue_fwd():
        with torch.no_grad():
            return composition(a, b, window, wts)

    def fused():
        a.grad = None
        loss = Lo.ms_ssim_loss(a, b, weights=weights)
        loss.backward()
        return loss.detach(), a.grad

    def glue():
        a.grad = None
        loss = composition(a, b, window, wts)
        loss.backward()
        return loss.detach(), a.grad
    lf, gf = (t.clone() for t in fused())
    lg, gg = (t.clone() for t in glue())
    r = dict(shape=list(shape), scales=scales, loss_abs_diff=abs(float(lf) - float(lg)),
             grad_max_rel_diff=float((gf - gg).abs().max() / gg.abs().max()))
    r['forward'] = measure(G, fused_fwd, glue_fwd, reps)
    r['forward_backward'] = measure(G, fused, glue, reps)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ms_ssim_probe.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('probe_ms_ssim: no GPU: nothing is measured without one')
    if args.reps < 200:
        print('probe_ms_ssim: fewer than 200 repetitions: a rehearsal, not a measurement')
    res = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, reps=args.reps,
               note='median of per-repetition device-event times; facts to record, not a condition',
               cases=[case(s, m, args.reps) for s, m in CASES])
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))
    for c in res['cases']:
        for what in ('forward', 'forward_backward'):
            m = c[what]
            line = 'ms_ssim_loss %s M %d %-16s: eager fused %8.1f us torch %8.1f us (%.2fx)' % (
                tuple(c['shape']), c['scales'], what, m['eager']['fused']['median_us'], m['eager']['torch']['median_us'],
                m['eager']['torch_over_fused'])
            line += '   graph'
            for k in ('fused', 'torch'):
                line += (' %s %8.1f us' % (k, m['graph'][k]['median_us']) if k in m['graph']
                         else ' %s not captured (%s)' % (k, m['graph'][k + '_error']))
            if 'torch_over_fused' in m['graph']:
                line += ' (%.2fx)' % m['graph']['torch_over_fused']
            print(line)
        print('   loss diff %.2g, grad rel diff %.2g' % (c['loss_abs_diff'], c['grad_max_rel_diff']))


if __name__ == '__main__':
    main()
