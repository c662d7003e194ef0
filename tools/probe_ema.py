"""fused weight EMA (ema.WeightEMA.update(), csrc/optim.hip) beside torch's multi-tensor lerp, in one process:
python tools/probe_ema.py [--reps 200] [--out profiles/ema_probe.json]

Device time on the real parameter lists of the x2 generator (Generator(16, 64, 256, [2]): 156 tensors, 1.39 M elements) and of the
96^2 discriminator (23.6 M elements: 283 MB of traffic at 12 bytes per element -- shadow read, parameter read, shadow write):
  fused        sisr_ema_prepare + sisr_ema_update over exactly that list (a WeightEMA over a holder of the parameters alone);
  torch_a/_b   torch._foreach_lerp_(shadows, params, 1 - d) over the same list, measured TWICE in the same alternation: the
               difference of its two medians is the run-to-run spread of this run;
  fused_net    WeightEMA.update() over the whole network as a trainer calls it (its buffers ride along: fp32 ones in the same
               launch, num_batches_tracked through one torch._foreach_copy_) -- for the record, not part of the condition.
Every variant is replayed from a HIP graph (device time, no launch gaps); after a warm-up the variants alternate, every
repetition between its own pair of device events; medians are reported.
Condition: fused <= torch + torch's spread, on both lists.
Refuses to run without a GPU."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

FEATS, STRIDES = [64, 64, 128, 128, 256, 256, 512, 512], [1, 2, 1, 2, 1, 2, 1, 2]      # config.py:81-82
HBM_PEAK = 8.0e12
DECAY = 0.999


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


def device_case(name, net, reps):
    from gpu_helpers import pkg
    G, ema = pkg('graph'), pkg('ema')
    params = list(net.parameters())
    numel = sum(p.numel() for p in params)
    holder = torch.nn.Module()
    holder.ps = torch.nn.ParameterList(params)
    fused, fused_net = ema.WeightEMA(holder, decay=DECAY), ema.WeightEMA(net, decay=DECAY)
    assert fused._n == len(params) and not fused._other
    gen = torch.Generator(device='cuda').manual_seed(1)
    shadows = [p.detach().clone() + torch.randn(p.shape, device='cuda', generator=gen) * 1e-3 for p in params]
    live = [p.detach() for p in params]
    graphs = dict(fused=G.GraphedStep(fused.update), fused_net=G.GraphedStep(fused_net.update),
                  torch=G.GraphedStep(lambda: torch._foreach_lerp_(shadows, live, 1.0 - DECAY)))
    variants = dict(torch_a=graphs['torch'], fused=graphs['fused'], torch_b=graphs['torch'], fused_net=graphs['fused_net'])
    t = {k: statistics.median(v) for k, v in alternate(variants, reps).items()}
    ref = 0.5 * (t['torch_a'] + t['torch_b'])
    spread = abs(t['torch_a'] - t['torch_b'])
    nbytes = 12 * numel
    rate = nbytes / (t['fused'] * 1e-6)
    return dict(net=name, tensors=len(params), numel=numel, bytes=nbytes, median_us={k: round(v, 2) for k, v in t.items()},
                torch_us=round(ref, 2), torch_spread_us=round(spread, 2), fused_minus_torch_us=round(t['fused'] - ref, 2),
                fused_bytes_per_s_T=round(rate / 1e12, 3), fused_share_of_hbm_peak=round(rate / HBM_PEAK, 3),
                torch_bytes_per_s_T=round(nbytes / (ref * 1e-6) / 1e12, 3), tensors_with_buffers=fused_net._n + len(fused_net._other),
                condition_met=bool(t['fused'] <= ref + spread))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ema_probe.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('probe_ema: no GPU: nothing is measured without one')
    if args.reps < 200:
        print('probe_ema: fewer than 200 repetitions: a rehearsal, not a measurement')
    from gpu_helpers import pkg
    mg, md = pkg('model_generator'), pkg('model_discriminator')
    torch.manual_seed(0)
    nets = (('generator_x2', mg.Generator(16, 64, 256, [2], use_sn=True).cuda()),
            ('discriminator_96', md.Discriminator((3, 96, 96), FEATS, STRIDES).cuda()))
    res = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, reps=args.reps, decay=DECAY,
               condition='fused (prepare + update) <= torch._foreach_lerp_ + its spread (medians of per-repetition device-event '
                         'times, graph replays; spread = difference of the two torch medians of the same alternation)',
               hbm_peak_bytes_per_s=HBM_PEAK, device_time=[device_case(name, net, args.reps) for name, net in nets])
    res['condition_met'] = all(c['condition_met'] for c in res['device_time'])
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))
    for c in res['device_time']:
        m = c['median_us']
        print('%-17s %4d tensors %9d elements: torch %.1f / %.1f us (%.2f TB/s)  fused %.1f us (%.2f TB/s, %.0f%% of the HBM peak)  '
              'fused - torch %.2f us, allowed %.2f us;  whole net (%d tensors) %.1f us' % (
                  c['net'], c['tensors'], c['numel'], m['torch_a'], m['torch_b'], c['torch_bytes_per_s_T'], m['fused'],
                  c['fused_bytes_per_s_T'], 100 * c['fused_share_of_hbm_peak'], c['fused_minus_torch_us'], c['torch_spread_us'],
                  c['tensors_with_buffers'], m['fused_net']))
    print('condition %s' % ('met' if res['condition_met'] else 'NOT met'))


if __name__ == '__main__':
    main()
