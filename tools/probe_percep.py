"""The multi-tap perceptual + Gram style loss (losses.perceptual_loss, csrc/percep.hip) beside the torch-op
composition of the same definition, in one process:  python tools/probe_percep.py [--reps 50] [--out profiles/percep_probe.json]

Shapes: the four taps of MaskedVGG(0b01111) at B16 / HR 96^2 (70.8 MB per feature tensor) and the five taps of the Real-ESRGAN setting
(MaskedVGG(0b11111), weights 0.1, 0.1, 1, 1, 1) at B16 / HR 192^2 (288 MB per feature tensor; skipped when the device has less than
16 GB free).  Criterion 'l1', the style term off and on.  Variants, alternated after 10 warm-up rounds, every repetition between its
own pair of device events, medians reported, as eager launches and as graph replays (graph.GraphedStep):
  fused_fwd / fused_fwd_bwd   perceptual_loss, and its backward pass through autograd (the gradient of fa: the generator's side);
  torch_fwd / torch_fwd_bwd   BasicSR's text on the same tensors: per tap a slice, a view, l1_loss, and for the style term
                              bmm(F, F^T) / (C H W) of both inputs and l1_loss of the two; and its backward pass.
The reference is torch, never the code under test.  gram_matrix of one input (the Gram launch and its reduction) is timed alone and
reported as a share of the 157.3 TFLOP/s fp32-matrix peak, counting 2 C^2 P FLOP per tap and sample (the kernel computes the
tiles on or above the diagonal only, so it executes about (T + 1) / (2 T) of that count per tap of T channel tiles).  Times are
reported, not asserted.  Refuses to run without a GPU."""
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
    ('mask01111_B16_HR96', 16, ((64, 96, 96), (128, 48, 48), (256, 24, 24), (512, 12, 12)), (1.0, 1.0, 1.0, 1.0)),
    ('realesrgan_mask11111_B16_HR192', 16, ((64, 192, 192), (128, 96, 96), (256, 48, 48), (512, 24, 24), (512, 12, 12)),
     (0.1, 0.1, 1.0, 1.0, 1.0)),
)


def composition(fa, fb, shapes, weights, style_weight):
    """BasicSR's PerceptualLoss.forward on the taps of two (B, total) tensors, criterion l1 -> percep (+ style)"""
    loss, off = 0, 0
    for (c, h, w), lw in zip(shapes, weights):
        x = fa[:, off:off + c * h * w].view(-1, c, h, w)
        y = fb[:, off:off + c * h * w].view(-1, c, h, w)
        off += c * h * w
        loss = loss + F.l1_loss(x, y) * lw
        if style_weight:
            fx, fy = x.view(-1, c, h * w), y.view(-1, c, h * w)
            gx, gy = fx.bmm(fx.transpose(1, 2)) / (c * h * w), fy.bmm(fy.transpose(1, 2)) / (c * h * w)
            loss = loss + style_weight * F.l1_loss(gx, gy) * lw
    return loss


def variants_for(b, shapes, weights, style_weight, Lm):
    total = sum(c * h * w for c, h, w in shapes)
    gen = torch.Generator(device='cuda').manual_seed(1)
    fb = torch.rand((b, total), device='cuda', generator=gen)                      # post-ReLU features are not negative
    fa = (fb + 0.1 * torch.randn((b, total), device='cuda', generator=gen)).clamp_min_(0).requires_grad_(True)

    def fused(a):
        percep, style = Lm.perceptual_loss(a, fb, shapes, weights, 1.0, style_weight, 'l1')
        return percep if style is None else percep + style

    def composed(a):
        return composition(a, fb, shapes, weights, style_weight)

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
    out = dict(fused_fwd=nograd(fused), torch_fwd=nograd(composed), fused_fwd_bwd=bwd(fused), torch_fwd_bwd=bwd(composed))
    if style_weight:
        out['fused_gram_one_input'] = lambda: Lm.gram_matrix(fb, shapes)
    return out


def ratios(m):
    """fused / composition for every pair that was timed"""
    for op in ('fwd', 'fwd_bwd'):
        if 'fused_' + op in m and 'torch_' + op in m:
            m['fused_%s_over_torch_%s' % (op, op)] = round(m['fused_' + op] / m['torch_' + op], 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'percep_probe.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('probe_percep: no GPU: nothing is measured without one')
    if args.reps < 20:
        print('probe_percep: fewer than 20 repetitions: a rehearsal, not a measurement')
    from gpu_helpers import pkg
    Lm, G = pkg('losses'), pkg('graph')
    res = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, reps=args.reps, criterion='l1',
               timing='medians of per-repetition device-event times in microseconds, variants alternated after 10 warm-up rounds; eager '
                      'launches on one stream, then the same callables as graph.GraphedStep replays',
               composition="BasicSR's PerceptualLoss.forward in torch ops on the same (B, total) tensors: per tap a slice, a view, "
                           'F.l1_loss, and with the style term bmm(F, F^T) / (C H W) of both inputs and F.l1_loss of the two',
               gram_flop='sum over taps of B 2 C^2 P, one input; the share is that count over the time of gram_matrix (the Gram '
                         'launch and its reduction) against %.1f TFLOP/s' % PEAK_F32_MATRIX_TFLOPS,
               settings={})
    for name, b, shapes, weights in SETTINGS:
        total = sum(c * h * w for c, h, w in shapes)
        if torch.cuda.mem_get_info()[0] < 40 * 4 * b * total:
            res['settings'][name] = dict(skipped='not enough free device memory')
            continue
        setting = dict(feature_tensor_bytes=4 * b * total, gram_flop_one_input=sum(b * 2 * c * c * h * w for c, h, w in shapes))
        for label, sw in (('style_off', 0.0), ('style_on', 1.0)):
            variants = variants_for(b, shapes, weights, sw, Lm)
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
                if 'fused_gram_one_input' in entry[mode]:
                    tflops = setting['gram_flop_one_input'] / entry[mode]['fused_gram_one_input'] * 1e-6
                    entry[mode]['gram_TFLOPs'] = round(tflops, 2)
                    entry[mode]['gram_share_of_fp32_matrix_peak'] = round(tflops / PEAK_F32_MATRIX_TFLOPS, 4)
            setting[label] = entry
            print(json.dumps({name + ' ' + label: entry}), flush=True)
            del variants, graphed
            torch.cuda.empty_cache()
        res['settings'][name] = setting
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
