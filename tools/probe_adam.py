"""capturable fused Adam (optim.Adam(capturable=True), csrc/optim.hip) beside the host-state step it extends, in one process:
python tools/probe_adam.py [--reps 200] [--iters 50] [--out profiles/adam_probe.json]

1. Device time on the real parameter lists of the x2 generator (Generator(16, 64, 256, [2])) and of the 96^2 discriminator: the
   parent path's sisr_adam_step (measured TWICE in the same alternation: the difference of its two medians is the run-to-run
   spread of this run), the capturable sequence prepare + step, the same with both guards (sum of squares + prepare + step), and
   the prepare launch alone.  Every variant is replayed from a HIP graph (device time, no launch gaps); after a warm-up the
   variants alternate, every repetition between its own pair of device events; medians are reported.
   Condition: capturable - parent <= parent's spread + prepare; guarded / parent ~ 8/7 (one more read of
   the gradients over the parent's 7 x 4 bytes per parameter).
2. Host time per cfg2-shaped iteration (bf16 build, B 16, HR 96^2, VGG22 content loss): the iteration as two replayed segments
   with od.step() between them and og.step() behind them on the host, against ONE graph with both capturable steps inside.
   Host time = wall clock to ISSUE an iteration (no synchronisation inside the loop); the total with the final synchronisation
   is reported beside it.
Refuses to run without a GPU."""
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

FEATS, STRIDES = [64, 64, 128, 128, 256, 256, 512, 512], [1, 2, 1, 2, 1, 2, 1, 2]      # config.py:81-82


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
    op, G, E, L = pkg('optim'), pkg('graph'), pkg('engine'), pkg('_lib')
    params = [p for p in net.parameters()]
    gen = torch.Generator(device='cuda').manual_seed(1)
    for p in params:
        p.grad = torch.randn(p.shape, device='cuda', generator=gen) * 1e-3
    numel = sum(p.numel() for p in params)
    opts = dict(parent=op.Adam(params, lr=1e-5), capturable=op.Adam(params, lr=1e-5, capturable=True),
                guarded=op.Adam(params, lr=1e-5, max_grad_norm=1.0, skip_nonfinite=True))
    graphs = {k: G.GraphedStep(o.step) for k, o in opts.items()}
    cap = opts['capturable']
    table, d, n = cap._tables[0], cap._dev, len(params)
    lr = d['lr'][0]

    def prepare_only():
        L.check(L.lib().sisr_adam_prepare(table[1].data_ptr() + 48 * n, n, lr.data_ptr(), 1, 0.9, 0.999, None, 0, -1.0, 0, 1,
                                          d['ctrl'].data_ptr(), d['consts'][0].data_ptr(), E._stream()), 'sisr_adam_prepare')
    graphs['prepare'] = G.GraphedStep(prepare_only)
    variants = dict(parent_a=graphs['parent'], capturable=graphs['capturable'], guarded=graphs['guarded'],
                    parent_b=graphs['parent'], prepare=graphs['prepare'])
    t = {k: statistics.median(v) for k, v in alternate(variants, reps).items()}
    parent = 0.5 * (t['parent_a'] + t['parent_b'])
    spread = abs(t['parent_a'] - t['parent_b'])
    r = dict(net=name, tensors=n, numel=numel, median_us={k: round(v, 2) for k, v in t.items()},
             parent_us=round(parent, 2), parent_spread_us=round(spread, 2),
             capturable_excess_us=round(t['capturable'] - parent, 2), allowed_excess_us=round(spread + t['prepare'], 2),
             guarded_over_parent=round(t['guarded'] / parent, 3), bytes_ratio_expected=round(8 / 7, 3),
             parent_bytes_per_s_T=round(7 * 4 * numel / (parent * 1e-6) / 1e12, 3))
    r['condition_met'] = bool(t['capturable'] - parent <= spread + t['prepare'])
    return r


def iteration_case(iters):
    from gpu_helpers import pkg
    E, G = pkg('engine'), pkg('graph')
    mg, md, mce, ut, op = (pkg('model_generator'), pkg('model_discriminator'), pkg('model_content_extractor'), pkg('utils'),
                           pkg('optim'))
    B, dev = 16, torch.device('cuda')
    E.set_precision('bf16')
    try:
        def setup(capturable):
            torch.manual_seed(0)
            net_g = mg.Generator(16, 64, 256, [2], use_sn=True).to(dev).train()
            net_d = md.Discriminator((3, 96, 96), FEATS, STRIDES).to(dev).train()
            ext = mce.MaskedVGG(0b00010, pretrained=False).to(dev)
            og = op.Adam(net_g.parameters(), lr=1e-5, capturable=capturable)
            od = op.Adam(net_d.parameters(), lr=1e-5, capturable=capturable)
            crit = torch.nn.BCELoss()
            hr = (torch.rand((B, 3, 96, 96), generator=torch.Generator().manual_seed(51)) * 2 - 1).cuda()
            ones, red, zeros = torch.ones(B, device=dev), torch.full((B,), .9, device=dev), torch.zeros(B, device=dev)

            def both():
                lr = ut.lr_from_hr(hr, (48, 48), device=dev)
                fake = net_g(lr)
                net_d.zero_grad()
                err_d = crit(net_d(hr).view(-1), red) + crit(net_d(fake.detach()).view(-1), zeros)
                err_d.backward()
                if capturable or not G.segment_boundary('d_step'):
                    od.step()
                net_g.zero_grad()
                err_g = crit(net_d(fake).view(-1), ones) * 5e-2 + torch.mean(torch.pow(ext(hr) - ext(fake), 2))
                err_g.backward()
                if capturable:
                    og.step()
                return err_d, err_g
            return og, od, both
        og, od, both = setup(False)
        seg = G.GraphedStep(both, between=lambda tag: od.step() if tag == 'd_step' else None)

        def segmented():
            seg()
            og.step()
        _, _, both1 = setup(True)
        one = G.GraphedStep(both1)
        out = {}
        for name, fn, graphs in (('segmented_host_steps', segmented, len(seg.graphs)), ('one_graph', one, len(one.graphs))):
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            out[name] = dict(graphs=graphs, host_us_per_iteration=round((t1 - t0) / iters * 1e6, 1),
                             wall_us_per_iteration=round((t2 - t0) / iters * 1e6, 1))
        return out
    finally:
        E.set_precision('fp32')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'adam_probe.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('probe_adam: no GPU: nothing is measured without one')
    if args.reps < 200:
        print('probe_adam: fewer than 200 repetitions: a rehearsal, not a measurement')
    from gpu_helpers import pkg
    mg, md = pkg('model_generator'), pkg('model_discriminator')
    torch.manual_seed(0)
    nets = (('generator_x2', mg.Generator(16, 64, 256, [2], use_sn=True).cuda()),
            ('discriminator_96', md.Discriminator((3, 96, 96), FEATS, STRIDES).cuda()))
    res = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, reps=args.reps, iters=args.iters,
               condition='capturable - parent <= parent spread + prepare (medians of per-repetition device-event times, graph replays)',
               device_time=[device_case(name, net, args.reps) for name, net in nets])
    del nets
    torch.cuda.empty_cache()
    res['iteration'] = iteration_case(args.iters)
    res['condition_met'] = all(c['condition_met'] for c in res['device_time'])
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))
    for c in res['device_time']:
        m = c['median_us']
        print('%-17s %4d tensors %9d elements: parent %.1f / %.1f us (%.2f TB/s)  capturable %.1f us  guarded %.1f us (%.3fx, bytes %.3fx)  '
              'prepare %.1f us  excess %.2f us, allowed %.2f us' % (
                  c['net'], c['tensors'], c['numel'], m['parent_a'], m['parent_b'], c['parent_bytes_per_s_T'], m['capturable'],
                  m['guarded'], c['guarded_over_parent'], c['bytes_ratio_expected'], m['prepare'], c['capturable_excess_us'],
                  c['allowed_excess_us']))
    for k, v in res['iteration'].items():
        print('%-22s %d graph(s): host %.1f us / iteration, wall %.1f us / iteration' % (
            k, v['graphs'], v['host_us_per_iteration'], v['wall_us_per_iteration']))
    print('condition %s' % ('met' if res['condition_met'] else 'NOT met'))


if __name__ == '__main__':
    main()
