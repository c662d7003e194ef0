"""the device-resident patch source (patches.DevicePatchSource, csrc/patchsrc.hip) beside the host-fed input path, in one process:
python tools/probe_patchsrc.py [--reps 200] [--out profiles/patchsrc_probe.json]

One batch of 16 HR 96 / LR 48 pairs out of a 64-image stand-in dataset of CelebA's decoded size (218 x 178 x 3 uint8):
  host_a/_b      the fastest input path without the source: a PINNED host uint8 batch, one asynchronous host-to-device copy, then
                 PatchPipeline((96, 96), (48, 48)) -- measured TWICE in the same alternation: the difference of its two medians
                 is the run-to-run spread of this run.  The host gather that fills the pinned batch is NOT in it;
  resize         DevicePatchSource(crop=None, resize=(96, 96), order='sequential'): the same output, sampled on the device;
  crop           DevicePatchSource(crop=(96, 96), hflip=True): random crops and flips, no resize;
  resize_graph / crop_graph   the same two replayed from a graph.GraphedStep.
After a warm-up the variants alternate, every repetition between its own pair of device events; medians are reported.  The outputs
of host and resize are compared bit for bit first.  Facts for DESIGN.md section 12, not a condition.  Refuses to run without a GPU."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from probe_ema import alternate  # noqa: E402

B, M, SHAPE, HR, LR = 16, 64, (218, 178, 3), (96, 96), (48, 48)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'patchsrc_probe.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('probe_patchsrc: no GPU: nothing is measured without one')
    if args.reps < 200:
        print('probe_patchsrc: fewer than 200 repetitions: a rehearsal, not a measurement')
    from gpu_helpers import pkg
    P, G = pkg('patches'), pkg('graph')
    gen = torch.Generator().manual_seed(3)
    host = torch.randint(0, 256, (M,) + SHAPE, dtype=torch.uint8, generator=gen)
    dataset = host.cuda()
    pinned = host[:B].clone().pin_memory()
    staged = torch.empty_like(pinned, device='cuda')
    pipe = P.PatchPipeline(HR, LR)

    def host_path():
        staged.copy_(pinned, non_blocking=True)
        return pipe(staged)

    resize = P.DevicePatchSource(dataset, B, LR, crop=None, resize=HR, order='sequential')
    crop = P.DevicePatchSource(dataset, B, LR, crop=HR, hflip=True, seed=1)
    want, got = host_path(), resize()                       # step 0 of the sequential order: images 0 .. 15
    torch.cuda.synchronize()
    same = bool(torch.equal(want[0], got[0]) and torch.equal(want[1], got[1]))
    resize_graph = G.GraphedStep(lambda: resize())
    crop_graph = G.GraphedStep(lambda: crop())
    variants = dict(host_a=host_path, resize=resize, crop=crop, resize_graph=resize_graph, host_b=host_path, crop_graph=crop_graph)
    t = {k: statistics.median(v) for k, v in alternate(variants, args.reps).items()}
    res = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, reps=args.reps, batch=B, dataset=[M] + list(SHAPE),
               hr=list(HR), lr=list(LR), host_and_resize_outputs_bit_equal=same,
               what='medians of per-repetition device-event times in microseconds, variants alternating in one process',
               median_us={k: round(v, 2) for k, v in t.items()}, host_us=round(0.5 * (t['host_a'] + t['host_b']), 2),
               host_spread_us=round(abs(t['host_a'] - t['host_b']), 2), h2d_bytes_per_batch=pinned.numel(),
               steps_drawn=dict(resize=int(resize.step_count), crop=int(crop.step_count)))
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))
    if not same:
        sys.exit('probe_patchsrc: the host-fed path and the device source disagree on the same images')


if __name__ == '__main__':
    main()
