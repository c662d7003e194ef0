"""NIQE on the device (metrics.niqe, csrc/niqe.hip) beside a torch-op composition of the same definition on the
device and the float64 NumPy restatement on the host, in one process:
    python tools/probe_niqe.py [--reps 200] [--out profiles/niqe_probe.json]

Shapes: (1, 3, 1152, 1536) -- one 2K validation image, 192 blocks -- and (16, 3, 192, 192) -- a validation batch of HR patches, 4
blocks each -- at block 96.  Variants, alternated after 10 warm-up rounds, every repetition between its own pair of device events,
medians reported, as eager launches and as graph replays (graph.GraphedStep):
  fused   metrics.niqe: five launches;
  torch   the same definition from torch ops in float64: the 7 x 7 windows by conv2d over a replicate-padded plane (raw moments, as
          upstream writes them; shifted slices where conv2d takes no float64), the down-scaling by index gathers, the blocks by
          unfold, the five fields of all blocks at once, the table search as a broadcast argmin over [fits, 9801], batched covariance
          and torch.linalg.solve.
The host restatement (tests/niqe_cases.py: features64 + score64) is timed once per shape with a wall clock, its input already on the
host: what a validation loop pays today on top of a device -> host copy.  The model is niqe_cases.model_for of the restatement's own
features.  Times are reported, not asserted; the three scores are printed beside them.  Refuses to run without a GPU."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from probe_degrade import alternate  # noqa: E402

SHAPES, BLOCK = ((1, 3, 1152, 1536), (16, 3, 192, 192)), 96


class Composition:
    """the definition from torch ops on the device, float64; NaN-free blocks are assumed (the probe's images have grain everywhere)"""

    def __init__(self, K, mu_p, cov_p, device):
        self.K = K
        g = torch.from_numpy(K.window()).to(device)
        self.g = g
        self.k2d = torch.outer(g, g).view(1, 1, 7, 7)
        self.taps = torch.from_numpy(K.HALF_TAPS).to(device)
        alpha, g1, g2, g3, rho = (torch.from_numpy(t).to(device) for t in K.tables())
        self.alpha, self.g1, self.g2, self.g3, self.rho = alpha, g1, g2, g3, rho
        self.mu_p, self.cov_p = torch.from_numpy(mu_p).to(device), torch.from_numpy(cov_p).to(device)
        self.index = {}
        self.windows = 'conv2d'
        try:
            self.blur(torch.zeros(1, 1, 8, 8, dtype=torch.float64, device=device))
        except RuntimeError:
            self.windows = 'shifted slices'

    def blur(self, p):
        pad = F.pad(p, (3, 3, 3, 3), mode='replicate')
        if self.windows == 'conv2d':
            return F.conv2d(pad, self.k2d)
        h, w = p.shape[2:]
        rows = sum(self.g[k] * pad[:, :, :, k:k + w] for k in range(7))
        return sum(self.g[k] * rows[:, :, k:k + h, :] for k in range(7))

    def mscn(self, p):
        mu = self.blur(p)
        sigma = torch.sqrt(torch.abs(self.blur(p * p) - mu * mu))
        return (p - mu) / (sigma + 1.0)

    def half(self, p):
        key = tuple(p.shape[2:])
        if key not in self.index:
            self.index[key] = tuple(torch.from_numpy(self.K.half_index(L)).to(p.device) for L in key)
        iy, ix = self.index[key]
        rows = sum(self.taps[k] * p[:, :, iy[k], :] for k in range(8))
        return sum(self.taps[k] * rows[:, :, :, ix[k]] for k in range(8))

    def features(self, m, B):
        blk = m.unfold(2, B, B).unfold(3, B, B).reshape(-1, B, B)
        f = torch.stack([blk] + [blk * torch.roll(blk, s, dims=(1, 2)) for s in self.K.SHIFTS]).flatten(2)      # [5, NB, B B]
        f2, neg, pos = f * f, f < 0, f > 0
        L = torch.sqrt((f2 * neg).sum(-1) / neg.sum(-1))
        R = torch.sqrt((f2 * pos).sum(-1) / pos.sum(-1))
        gam = L / R
        r = f.abs().mean(-1) ** 2 / f2.mean(-1)
        rhat = r * (gam ** 3 + 1) * (gam + 1) / (gam ** 2 + 1) ** 2
        j = torch.argmin((self.rho - rhat.unsqueeze(-1)) ** 2, dim=-1)                                          # [5, NB, 9801]
        t = torch.sqrt(self.g1[j] / self.g3[j])
        bl, br = L * t, R * t
        m_ = (br - bl) * (self.g2[j] / self.g1[j])
        a = self.alpha[j]
        cols = [a[0], (bl[0] + br[0]) / 2]
        for k in range(1, 5):
            cols += [a[k], m_[k], bl[k], br[k]]
        return torch.stack(cols, dim=-1)                                                                        # [NB, 18]

    def __call__(self, img):
        n = img.shape[0]
        v = (img.double() + 1.0) * 127.5
        y = torch.round(16.0 + ((65.481 * v[:, 0] + 128.553 * v[:, 1]) + 24.966 * v[:, 2]) / 255.0).unsqueeze(1)
        y = y[:, :, :y.shape[2] // BLOCK * BLOCK, :y.shape[3] // BLOCK * BLOCK]
        feat = torch.cat([self.features(self.mscn(y), BLOCK), self.features(self.mscn(self.half(y)), BLOCK // 2)], dim=-1).view(n, -1, 36)
        mu = feat.mean(dim=1)
        c = feat - mu.unsqueeze(1)
        cov = c.transpose(1, 2) @ c / (feat.shape[1] - 1)
        S, d = (self.cov_p + cov) / 2, (self.mu_p - mu).unsqueeze(-1)
        return torch.sqrt((d * torch.linalg.solve(S, d)).sum(dim=(1, 2))).float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'niqe_probe.json'))
    ap.add_argument('--no-host', action='store_true', help='skip the host restatement (it takes about a minute per shape)')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('probe_niqe: no GPU: nothing is measured without one')
    if args.reps < 200:
        print('probe_niqe: fewer than 200 repetitions: a rehearsal, not a measurement')
    import niqe_cases as K
    from gpu_helpers import pkg
    M, G = pkg('metrics'), pkg('graph')
    res = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, reps=args.reps, block=BLOCK,
               timing='medians of per-repetition device-event times in microseconds, variants alternated after 10 warm-up rounds; eager '
                      'launches on one stream, then the same callables as graph.GraphedStep replays; the host restatement once, wall clock',
               composition='float64 torch ops on the device: windows over a replicate-padded plane from raw moments, index gathers for the '
                           'down-scaling, unfold blocks, broadcast argmin over [fits, 9801], batched covariance, torch.linalg.solve',
               shapes={})
    for shape in SHAPES:
        img = (0.7 * K.natural(shape, 3, 0.25)).clamp(-1, 1)
        entry = {}
        if args.no_host:
            feat = M.niqe_features(img.cuda(), BLOCK).cpu().numpy()
        else:
            t0 = time.perf_counter()
            feat = K.features64(img, BLOCK)[0]
            t1 = time.perf_counter()
        mu_p, cov_p = K.model_for(feat)
        if not args.no_host:
            t2 = time.perf_counter()
            host = [K.score64(f, mu_p, cov_p) for f in feat]
            entry['host_numpy_seconds'] = round(t1 - t0 + time.perf_counter() - t2, 3)
            entry['host_scores'] = host[:4]
        model = M.NiqeModel(mu_p, cov_p, BLOCK).to('cuda')
        x = img.cuda()
        comp = Composition(K, mu_p, cov_p, x.device)
        entry['composition_windows'] = comp.windows
        variants = dict(fused=lambda: M.niqe(x, model), torch=lambda: comp(x))
        entry['fused_scores'], entry['torch_scores'] = variants['fused']().tolist()[:4], variants['torch']().tolist()[:4]
        t = alternate(variants, args.reps)
        entry['eager_median_us'] = {k: round(statistics.median(v), 2) for k, v in t.items()}
        graphed, failed = {}, {}
        for k, fn in variants.items():
            try:
                graphed[k] = G.GraphedStep(fn)
            except G.GraphCaptureError as e:
                failed[k] = str(e)[:300]
        if graphed:
            t = alternate(graphed, args.reps)
            entry['graph_median_us'] = {k: round(statistics.median(v), 2) for k, v in t.items()}
        if failed:
            entry['graph_capture_failed'] = failed
        for mode in ('eager_median_us', 'graph_median_us'):
            m = entry.get(mode, {})
            if 'fused' in m and 'torch' in m:
                m['fused_over_torch'] = round(m['fused'] / m['torch'], 4)
        res['shapes']['x'.join(str(v) for v in shape)] = entry
        print(json.dumps({str(shape): entry}), flush=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
