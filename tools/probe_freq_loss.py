"""fused frequency-domain loss (losses.frequency_loss, csrc/freq_loss.hip) beside the torch-op composition of the same definition,
in one process on the same tensors: python tools/probe_freq_loss.py [--reps 200] [--out profiles/freq_loss_probe.json]

Cases: 16 x 3 x 96 x 96 and 16 x 3 x 192 x 192 (the HR patches of the configs), kinds 'l1', 'charbonnier' and 'focal', the gradient
going to the fake side only, as in the G step.  The composition is the definition written with torch ops on the device
(torch.fft.rfft2 of each image for 'l1' / 'charbonnier', torch.fft.fft2(norm='ortho') of each image and the detached weight matrix
for 'focal', autograd backward).  Timed: the forward alone (under no_grad) and forward + backward.  After a warm-up the two variants
alternate, every repetition between its own pair of device events; the median is reported (and the mean).  Measured twice: launched
eagerly (host launch work included where the device outruns it) and replayed from a HIP graph of the same calls
(graph.GraphedStep: device time alone).  If a variant cannot be captured, that is recorded and the graphed comparison is left out.
These times are facts to record, not a condition: at these sizes the library FFT is a serious opponent.  Refuses to run without a
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

SHAPES = [(16, 3, 96, 96), (16, 3, 192, 192)]
KINDS = ['l1', 'charbonnier', 'focal']
EPS, ALPHA = 1e-3, 1.0


def composition(a, b, kind):
    """the definition with torch ops -> 0-dim loss (mean over the batch)"""
    if kind in ('l1', 'charbonnier'):
        D = torch.fft.rfft2(a) - torch.fft.rfft2(b)
        z = torch.view_as_real(D)
        rho = z.abs() if kind == 'l1' else torch.sqrt(z * z + EPS * EPS)
        return rho.mean(dim=(1, 2, 3, 4)).mean()
    D = torch.fft.fft2(a, norm='ortho') - torch.fft.fft2(b, norm='ortho')
    dist = D.real ** 2 + D.imag ** 2
    wt = torch.sqrt(dist) ** ALPHA
    wt = wt / wt.amax(dim=(2, 3), keepdim=True)
    wt = torch.nan_to_num(wt, nan=0.0).clamp(0, 1).detach()
    return (wt * dist).mean(dim=(1, 2, 3)).mean()


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


def case(shape, kind, reps):
    from gpu_helpers import pkg
    Lo, G = pkg('losses'), pkg('graph')
    a, b = batch(shape)
    kw = dict(kind=kind, eps=EPS, alpha=ALPHA)

    def fused_fwd():
        with torch.no_grad():
            return Lo.frequency_loss(a, b, **kw)

    def glue_fwd():
        with torch.no_grad():
            return composition(a, b, kind)

    def fused():
        a.grad = None
        loss = Lo.frequency_loss(a, b, **kw)
        loss.backward()
        return loss.detach(), a.grad

    def glue():
        a.grad = None
        loss = composition(a, b, kind)
        loss.backward()
        return loss.detach(), a.grad
    lf, gf = (t.clone() for t in fused())
    lg, gg = (t.clone() for t in glue())
    r = dict(shape=list(shape), kind=kind, loss_rel_diff=abs(float(lf) - float(lg)) / abs(float(lg)),
             grad_max_rel_diff=float((gf - gg).abs().max() / gg.abs().max()))
    r['forward'] = measure(G, fused_fwd, glue_fwd, reps)
    r['forward_backward'] = measure(G, fused, glue, reps)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'freq_loss_probe.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('probe_freq_loss: no GPU: nothing is measured without one')
    if args.reps < 200:
        print('probe_freq_loss: fewer than 200 repetitions: a rehearsal, not a measurement')
    res = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, reps=args.reps,
               note='median of per-repetition device-event times; facts to record, not a condition',
               cases=[case(s, k, args.reps) for s in SHAPES for k in KINDS])
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))
    for c in res['cases']:
        for what in ('forward', 'forward_backward'):
            m = c[what]
            line = 'frequency_loss %s %-11s %-16s: eager fused %8.1f us torch %8.1f us (%.2fx)' % (
                tuple(c['shape']), c['kind'], what, m['eager']['fused']['median_us'], m['eager']['torch']['median_us'],
                m['eager']['torch_over_fused'])
            line += '   graph'
            for k in ('fused', 'torch'):
                line += (' %s %8.1f us' % (k, m['graph'][k]['median_us']) if k in m['graph']
                         else ' %s not captured (%s)' % (k, m['graph'][k + '_error']))
            if 'torch_over_fused' in m['graph']:
                line += ' (%.2fx)' % m['graph']['torch_over_fused']
            print(line)
        print('   loss rel diff %.2g, grad rel diff %.2g' % (c['loss_rel_diff'], c['grad_max_rel_diff']))


if __name__ == '__main__':
    main()
