"""second-order degradation (degrade.HighOrderDegrader, csrc/degrade.hip) beside the torch-op composition of
the same definition, in one process:  python tools/probe_degrade_mix.py [--reps 200] [--out profiles/degrade_mix_probe.json]

Shape: (16, 3, 192, 192) -> middle (136, 136) -> (96, 96), the two published stages (K = 21, JPEG in both, final sinc filter) with a
FIXED middle size -- the x2 training batch.  Variants, alternated after a warm-up, every repetition between its own pair of device
events, medians reported, as eager launches and as a graph replay (graph.GraphedStep):
  fused_fwd / fused_fwd_bwd   HighOrderDegrader.__call__ (draws included) and its backward pass through autograd;
  torch_fwd / torch_fwd_bwd   per stage F.pad(replicate) + a grouped F.conv2d with per-sample weights, the package's bicubic kernel,
                              torch.randn noise of the same four kinds (per-sample mode and grey flag by torch.where), clamp, the
                              package's JPEG round trip; the final filter as pad + conv + clamp.  It draws nothing: it reuses the
                              tables of one fused call.
The launch count of the fused call is taken from the library calls of one forward + backward.  Times are reported, not asserted.
Refuses to run without a GPU."""
import argparse
import collections
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

SHAPE, MID, SIZE = (16, 3, 192, 192), (136, 136), (96, 96)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'degrade_mix_probe.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('probe_degrade_mix: no GPU: nothing is measured without one')
    if args.reps < 200:
        print('probe_degrade_mix: fewer than 200 repetitions: a rehearsal, not a measurement')
    from gpu_helpers import pkg
    D, U, J, G, L = pkg('degrade'), pkg('utils'), pkg('jpeg'), pkg('graph'), pkg('_lib')
    n, c, _, _ = SHAPE
    gen = torch.Generator(device='cuda').manual_seed(1)
    x = (2 * torch.rand(SHAPE, device='cuda', generator=gen) - 1).requires_grad_(True)
    dy = torch.randn((n, c) + SIZE, device='cuda', generator=gen)
    d = D.HighOrderDegrader(mid_size=MID, seed=1)
    luma = torch.tensor([0.299, 0.587, 0.114], device='cuda').view(1, 3, 1, 1)

    # the launches of one fused forward + backward, by the entry point behind each
    calls, check = collections.Counter(), L.check

    def counting(status, what):
        calls[what] += 1
        return check(status, what)
    L.check = counting
    try:
        x.grad = None
        d(x, SIZE).backward(dy)
    finally:
        L.check = check
    torch.cuda.synchronize()
    tables = [(k.clone(), nt.clone(), tb.clone(), sz) for k, nt, tb, sz in zip(d.last_kernels, d.last_noise_table, d.last_tables, d.last_sizes)]
    final = d.last_final_kernels.clone()

    def blur(inp, k):
        R = (k.shape[-1] - 1) // 2
        h, w = inp.shape[-2:]
        xp = F.pad(inp, (R, R, R, R), mode='replicate').reshape(1, n * c, h + 2 * R, w + 2 * R)
        return F.conv2d(xp, k.repeat_interleave(c, dim=0)[:, None], groups=n * c).reshape(n, c, h, w)

    def noise(inp, nt):
        mode, grey, amp = (nt[:, i].view(n, 1, 1, 1) for i in range(3))
        v = inp.detach()
        z = torch.where(grey > 0, torch.randn_like(v[:, :1]).expand_as(v), torch.randn_like(v))
        v = torch.where(grey > 0, (v * luma).sum(dim=1, keepdim=True).expand_as(v), v)
        shot = amp / 8 * ((v + 1) / 2).clamp(0, 1).sqrt()
        return (inp + torch.where(mode == 1, amp.expand_as(v), torch.where(mode == 2, shot, torch.zeros_like(v))) * z).clamp(-1, 1)

    def torch_fwd(inp=x):
        out = inp
        for i, (k, nt, tb, sz) in enumerate(tables):
            out = noise(U._subsampling_interpolation(blur(out, k), sz), nt)
            if i == len(tables) - 1:
                out = blur(out, final).clamp(-1, 1)
            out = J.jpeg_roundtrip(out, tb, d.jpeg_subsampling, d.jpeg_grad, True)
        return out

    def fused_fwd(inp=x):
        return d(inp, SIZE)

    def bwd(fwd):
        def run():
            x.grad = None
            fwd().backward(dy)
            return x.grad
        return run

    def nograd(fwd):
        def run():
            with torch.no_grad():
                return fwd(x.detach())
        return run
    variants = dict(torch_fwd=nograd(torch_fwd), fused_fwd=nograd(fused_fwd), torch_fwd_bwd=bwd(torch_fwd), fused_fwd_bwd=bwd(fused_fwd))
    res = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, reps=args.reps, shape=SHAPE, mid_size=MID, size=SIZE,
               stages='realesrgan_stages(): K = 21, JPEG 30-95 in both stages, final sinc filter with probability 0.8, sinc_jpeg order',
               timing='medians of per-repetition device-event times, variants alternated after 10 warm-up rounds; eager launches on one '
                      'stream, then the same four callables as graph.GraphedStep replays',
               fused_launches_fwd_bwd=dict(calls), fused_launches_total=sum(calls.values()))
    t = alternate(variants, args.reps)
    res['eager_median_us'] = {k: round(statistics.median(v), 2) for k, v in t.items()}
    try:
        graphed = {k: G.GraphedStep(fn) for k, fn in variants.items()}
    except G.GraphCaptureError as e:
        res['graph_median_us'] = dict(error=str(e))
    else:
        t = alternate(graphed, args.reps)
        res['graph_median_us'] = {k: round(statistics.median(v), 2) for k, v in t.items()}
    for mode in ('eager_median_us', 'graph_median_us'):
        m = res[mode]
        if 'error' not in m:
            m['fused_over_torch_fwd'] = round(m['fused_fwd'] / m['torch_fwd'], 4)
            m['fused_over_torch_fwd_bwd'] = round(m['fused_fwd_bwd'] / m['torch_fwd_bwd'], 4)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
