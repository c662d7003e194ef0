"""fused image-space loss (losses.image_loss, csrc/image_loss.hip) beside the torch-op composition of the same definition, forward +
backward, in one process on the same tensors: python tools/probe_image_loss.py [--reps 200] [--out profiles/image_loss_probe.json]

The loss is ssim_weight = 1, pixel_weight = 1, pixel = 'charbonnier' on 16 x 3 x 96 x 96 and 16 x 3 x 192 x 192 batches (the HR
patches of the configs), the gradient going to the fake side only, as in the G step.  The composition is the definition written
with torch ops: ten single-channel F.conv2d windows (11 x 1 then 1 x 11 for each of a, b, a^2, b^2, ab), the SSIM map and the
Charbonnier term elementwise, autograd backward.  After a warm-up the two variants alternate, every repetition between its own pair
of device events; the median is reported (and the mean).  Measured twice: launched eagerly (host launch work included where the
device outruns it) and replayed from a HIP graph of the same calls (graph.GraphedStep: device time alone).  If the composition
cannot be captured, that is recorded and the graphed comparison is left out.
Condition (both sizes, every way of launching that was measured): fused time <= composition time.  Refuses to run without a GPU.
Per-kernel times come from a separate run under rocprofv3 --kernel-trace --stats: --trace-size 192 launches the fused forward +
backward alone, 50 times at 16 x 3 x 192 x 192, and measures nothing itself."""
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

SIZES = [(16, 3, 96, 96), (16, 3, 192, 192)]
KW = dict(ssim_weight=1.0, pixel_weight=1.0, pixel='charbonnier', eps=1e-3)
WINDOW, DATA_RANGE = 11, 2.0


def composition(a, b, window):
    """the definition with torch ops -> 0-dim loss (mean over the batch)"""
    n, c, h, w = a.shape

    def win(t):
        t = t.reshape(n * c, 1, h, w)
        return F.conv2d(F.conv2d(t, window.view(1, 1, WINDOW, 1)), window.view(1, 1, 1, WINDOW))
    c1, c2 = (0.01 * DATA_RANGE) ** 2, (0.03 * DATA_RANGE) ** 2
    mu_a, mu_b = win(a), win(b)
    var_a, var_b, cov = win(a * a) - mu_a ** 2, win(b * b) - mu_b ** 2, win(a * b) - mu_a * mu_b
    m = ((2 * mu_a * mu_b + c1) * (2 * cov + c2)) / ((mu_a ** 2 + mu_b ** 2 + c1) * (var_a + var_b + c2))
    ssim = m.reshape(n, -1).mean(dim=1)
    d = a - b
    pix = torch.sqrt(d * d + KW['eps'] ** 2).mean(dim=(1, 2, 3))
    return (KW['ssim_weight'] * (1 - ssim) + KW['pixel_weight'] * pix).mean()


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


def trace(size, reps=50):
    from gpu_helpers import pkg
    Lo = pkg('losses')
    a, b = batch((16, 3, size, size))
    for _ in range(reps):
        a.grad = None
        Lo.image_loss(a, b, data_range=DATA_RANGE, **KW).backward()
    torch.cuda.synchronize()


def case(shape, reps):
    from gpu_helpers import pkg
    Lo, G = pkg('losses'), pkg('graph')
    a, b = batch(shape)
    window = torch.exp(-(torch.arange(WINDOW, dtype=torch.float64) - WINDOW // 2) ** 2 / (2 * 1.5 ** 2))
    window = (window / window.sum()).float().cuda()

    def fused():
        a.grad = None
        loss = Lo.image_loss(a, b, data_range=DATA_RANGE, **KW)
        loss.backward()
        return loss.detach(), a.grad

    def glue():
        a.grad = None
        loss = composition(a, b, window)
        loss.backward()
        return loss.detach(), a.grad
    lf, gf = (t.clone() for t in fused())
    lg, gg = (t.clone() for t in glue())
    r = dict(shape=list(shape), loss_abs_diff=abs(float(lf) - float(lg)), grad_max_rel_diff=float((gf - gg).abs().max() / gg.abs().max()))
    t = alternate(dict(fused=fused, torch=glue), reps)
    r['eager'] = {k: summary(v) for k, v in t.items()}
    try:
        variants = dict(fused=G.GraphedStep(fused), torch=G.GraphedStep(glue))
    except G.GraphCaptureError as e:
        r['graph'] = dict(error=str(e))
    else:
        t = alternate(variants, reps)
        r['graph'] = {k: summary(v) for k, v in t.items()}
    ok = True
    for mode in ('eager', 'graph'):
        if 'error' not in r[mode]:
            r[mode]['torch_over_fused'] = round(r[mode]['torch']['median_us'] / r[mode]['fused']['median_us'], 3)
            ok = ok and r[mode]['torch_over_fused'] >= 1.0
    r['fused_no_slower'] = ok
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'image_loss_probe.json'))
    ap.add_argument('--trace-size', type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('probe_image_loss: no GPU: nothing is measured without one')
    if args.trace_size:
        return trace(args.trace_size)
    if args.reps < 200:
        print('probe_image_loss: fewer than 200 repetitions: a rehearsal, not a measurement')
    res = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, reps=args.reps, loss=KW,
               condition='fused forward + backward <= torch-op composition (median of per-repetition device-event times)',
               cases=[case(s, args.reps) for s in SIZES])
    res['condition_met'] = all(c['fused_no_slower'] for c in res['cases'])
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))
    for c in res['cases']:
        line = 'image_loss %s: eager fused %8.1f us torch %8.1f us (%.2fx)' % (
            tuple(c['shape']), c['eager']['fused']['median_us'], c['eager']['torch']['median_us'], c['eager']['torch_over_fused'])
        if 'error' in c['graph']:
            line += '   graph: %s' % c['graph']['error']
        else:
            line += '   graph fused %8.1f us torch %8.1f us (%.2fx)' % (
                c['graph']['fused']['median_us'], c['graph']['torch']['median_us'], c['graph']['torch_over_fused'])
        print(line + '   loss diff %.2g, grad rel diff %.2g' % (c['loss_abs_diff'], c['grad_max_rel_diff']))
    print('condition %s' % ('met' if res['condition_met'] else 'NOT met'))


if __name__ == '__main__':
    main()
