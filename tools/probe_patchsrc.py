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
of host and resize are compared bit for bit first.  Facts for DESIGN.md section 12, not a condition.  Refuses to run without a GPU.

python tools/probe_patchsrc.py --ragged [--out profiles/patchsrc_ragged_probe.json]
the crop source over a packed store (patches.RaggedPatchSource) beside the uniform one, same batch and window, same alternation:
  crop_a/_b      DevicePatchSource(crop=(96, 96), hflip=True) as above, through sisr_patch_draw / sisr_patch_gather, twice;
  ragged_equal   RaggedPatchSource over the same 64 images packed one after the other;
  ragged_mixed   RaggedPatchSource over 64 images of mixed sizes (96 .. 351 pixels a side, the same number of images);
  crop_permuted / ragged_permuted   the first and the third in order='permuted' (24 rounds of the shuffle in the draw launch).
Two alternations: the six issued eagerly, then the same six replayed from a graph.GraphedStep each (a replay leaves the queue
empty behind it, which an eager variant next in turn would pay for).  The batches of crop and ragged_equal are compared bit for
bit first."""
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
    ap.add_argument('--out', default=None)
    ap.add_argument('--ragged', action='store_true')
    args = ap.parse_args()
    args.out = args.out or os.path.join(ROOT, 'profiles', 'patchsrc_ragged_probe.json' if args.ragged else 'patchsrc_probe.json')
    if not torch.cuda.is_available():
        sys.exit('probe_patchsrc: no GPU: nothing is measured without one')
    if args.reps < 200:
        print('probe_patchsrc: fewer than 200 repetitions: a rehearsal, not a measurement')
    from gpu_helpers import pkg
    P, G = pkg('patches'), pkg('graph')
    gen = torch.Generator().manual_seed(3)
    host = torch.randint(0, 256, (M,) + SHAPE, dtype=torch.uint8, generator=gen)
    dataset = host.cuda()
    if args.ragged:
        return ragged(args, P, G, host, dataset)
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


def ragged(args, P, G, host, dataset):
    sizes = [(96 + (37 * i) % 256, 96 + (91 * i) % 256) for i in range(M)]
    gen = torch.Generator().manual_seed(4)
    mixed = P.PackedImages.from_images([torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=gen) for h, w in sizes], 'cuda')
    equal = P.PackedImages.from_images(list(host), 'cuda')
    crop = lambda **kw: P.DevicePatchSource(dataset, B, LR, crop=HR, hflip=True, seed=1, **kw)
    rag = lambda store, **kw: P.RaggedPatchSource(store, B, LR, crop=HR, hflip=True, seed=1, **kw)
    a, b = crop()(), rag(equal)()
    torch.cuda.synchronize()
    same = bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]))
    make = lambda: dict(crop_a=crop(), ragged_equal=rag(equal), ragged_mixed=rag(mixed), crop_permuted=crop(order='permuted'),
                        ragged_permuted=rag(mixed, order='permuted'), crop_b=crop())
    med = lambda variants: {k: round(statistics.median(v), 2) for k, v in alternate(variants, args.reps).items()}
    eager = med(make())
    graph = med({k: G.GraphedStep(lambda src=src: src()) for k, src in make().items()})
    spread = lambda t: round(abs(t['crop_a'] - t['crop_b']), 2)
    res = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, reps=args.reps, batch=B, window=list(HR), lr=list(LR),
               uniform_dataset=[M] + list(SHAPE), mixed_sizes=dict(images=M, min=[min(s[0] for s in sizes), min(s[1] for s in sizes)],
                                                                  max=[max(s[0] for s in sizes), max(s[1] for s in sizes)],
                                                                  bytes=mixed.data.numel()),
               crop_and_ragged_equal_outputs_bit_equal=same,
               what='medians of per-repetition device-event times in microseconds; two alternations in one process: the variants '
                    'issued eagerly, then each replayed from a GraphedStep; crop_a and crop_b are the same source twice',
               eager_median_us=eager, eager_crop_spread_us=spread(eager), graph_median_us=graph, graph_crop_spread_us=spread(graph))
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))
    if not same:
        sys.exit('probe_patchsrc: the uniform and the packed source disagree on the same images')


if __name__ == '__main__':
    main()
