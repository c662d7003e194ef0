"""The contextual loss (losses.contextual_loss, csrc/contextual.hip) beside the torch-op composition of the same
definition, in one process:  python tools/probe_contextual.py [--reps 30] [--out profiles/contextual_probe.json]

Shapes: B16 with the MaskedVGG taps conv3_4 and conv4_4 at HR 96^2 (C 256 / 512, P 576 / 144), and with conv2_2 added (C 128, P 2304: the
cap, 340 MB of similarity).  Variants, alternated after 10 warm-up rounds, every repetition between its own pair of device events,
medians reported, as eager launches and as graph replays (graph.GraphedStep):
  fused_fwd / fused_fwd_bwd   contextual_loss, and its backward pass through autograd (the gradient of fa: the generator's side);
  torch_fwd / torch_fwd_bwd   the common PyTorch text on the same tensors: per tap y-mean centring, F.normalize, bmm, min over the
                              target axis, exp, the row normalisation, max over the source axis, log; and its backward pass.
The reference is torch, never the code under test.  The peak of the caching allocator above what is allocated before the call is
recorded for every variant (one call after the timing): the B P^2 intermediates are what the fused path does not keep.  The
similarity alone (contextual_similarity: mu, norms, the product) is timed and reported as a share of the 157.3 TFLOP/s fp32-matrix
peak, counting 2 P^2 C FLOP per tap and sample.  Times are reported, not asserted.  Refuses to run without a GPU."""
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

PEAK_F32_MATRIX_TFLOPS = 157.3
SETTINGS = (
    ('conv3_4_conv4_4_B16_HR96', 16, ((256, 24, 24), (512, 12, 12)), (1.0, 1.0)),
    ('conv2_2_conv3_4_conv4_4_B16_HR96', 16, ((128, 48, 48), (256, 24, 24), (512, 12, 12)), (1.0, 1.0, 1.0)),
)
BAND = 0.5


def composition(fa, fb, shapes, weights):
    """the cosine contextual loss in torch ops on the taps of two (B, total) tensors; fb is the target"""
    loss, off = 0, 0
    for (c, h, w), lw in zip(shapes, weights):
        x = fa[:, off:off + c * h * w].view(-1, c, h * w)
        y = fb[:, off:off + c * h * w].view(-1, c, h * w)
        off += c * h * w
        mu = y.mean(dim=(0, 2), keepdim=True)
        d = 1 - torch.bmm(F.normalize(x - mu, p=2, dim=1).transpose(1, 2), F.normalize(y - mu, p=2, dim=1))
        wgt = torch.exp((1 - d / (d.min(dim=2, keepdim=True)[0] + 1e-5)) / BAND)
        cx = wgt / wgt.sum(dim=2, keepdim=True)
        loss = loss + lw * (-torch.log(cx.max(dim=1)[0].mean(dim=1) + 1e-5)).mean()
    return loss


def variants_for(b, shapes, weights, Lm):
    total = sum(c * h * w for c, h, w in shapes)
    gen = torch.Generator(device='cuda').manual_seed(1)
    fb = torch.rand((b, total), device='cuda', generator=gen)                      # post-ReLU features are not negative
    fa = (fb + 0.5 * torch.randn((b, total), device='cuda', generator=gen)).clamp_min_(0).requires_grad_(True)

    def fused(a):
        return Lm.contextual_loss(a, fb, shapes, weights, BAND)

    def composed(a):
        return composition(a, fb, shapes, weights)

    def nograd(fn):
        def run():
            with torch.no_grad():
                return fn(fa.detach())
        return run

    def bwd(fn):
        def run():
            fa.grad = None
            fn(fa).backward()
            return fa.grad
        return run
    return dict(fused_fwd=nograd(fused), torch_fwd=nograd(composed), fused_fwd_bwd=bwd(fused), torch_fwd_bwd=bwd(composed),
                fused_similarity=lambda: Lm.contextual_similarity(fa, fb, shapes))


def peak_bytes(fn):
    """the allocator's peak during one call above what was allocated before it"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return int(peak)


def ratios(m):
    """fused / composition for every pair that was timed"""
    for op in ('fwd', 'fwd_bwd'):
        if 'fused_' + op in m and 'torch_' + op in m:
            m['fused_%s_over_torch_%s' % (op, op)] = round(m['fused_' + op] / m['torch_' + op], 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'contextual_probe.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('probe_contextual: no GPU: nothing is measured without one')
    if args.reps < 20:
        print('probe_contextual: fewer than 20 repetitions: a rehearsal, not a measurement')
    from gpu_helpers import pkg
    Lm, G = pkg('losses'), pkg('graph')
    res = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, reps=args.reps, band_width=BAND,
               timing='medians of per-repetition device-event times in microseconds, variants alternated after 10 warm-up rounds; eager '
                      'launches on one stream, then the same callables as graph.GraphedStep replays',
               composition='the common PyTorch text of the cosine contextual loss on the same (B, total) tensors: per tap y-mean '
                           'centring, F.normalize, bmm, min, exp, row normalisation, max, log',
               memory='peak of the caching allocator during one eager call above what was allocated before it, bytes',
               similarity_flop='sum over taps of B 2 P^2 C; the share is that count over the time of contextual_similarity (mu, norms '
                               'and the product) against %.1f TFLOP/s' % PEAK_F32_MATRIX_TFLOPS,
               settings={})
    for name, b, shapes, weights in SETTINGS:
        total = sum(c * h * w for c, h, w in shapes)
        sim_bytes = sum(4 * b * (h * w) ** 2 for _, h, w in shapes)
        if torch.cuda.mem_get_info()[0] < 24 * sim_bytes + 40 * 4 * b * total:
            res['settings'][name] = dict(skipped='not enough free device memory')
            continue
        entry = dict(feature_tensor_bytes=4 * b * total, similarity_bytes=sim_bytes,
                     similarity_flop=sum(b * 2 * c * (h * w) ** 2 for c, h, w in shapes))
        variants = variants_for(b, shapes, weights, Lm)
        t = alternate(variants, args.reps)
        entry['eager_median_us'] = {k: round(statistics.median(v), 2) for k, v in t.items()}
        entry['peak_bytes'] = {k: peak_bytes(fn) for k, fn in variants.items()}
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
            if 'fused_similarity' in entry[mode]:
                tflops = entry['similarity_flop'] / entry[mode]['fused_similarity'] * 1e-6
                entry[mode]['similarity_TFLOPs'] = round(tflops, 2)
                entry[mode]['similarity_share_of_fp32_matrix_peak'] = round(tflops / PEAK_F32_MATRIX_TFLOPS, 4)
        res['settings'][name] = entry
        print(json.dumps({name: entry}), flush=True)
        del variants, graphed
        torch.cuda.empty_cache()
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
