"""CPU, world_size 2 over gloo: the data-parallel gradient exchange used for N > 1 (the RCCL path
differs only in backend and streams).
  * post-backward form: each rank holds a different gradient; after the exchange both hold the mean;
  * bucket-ready form (what the generator's backward schedule drives, generator_engine.run_backward): every
    rank computes the ORACLE's gradients on its half of one golden batch (per-replica BatchNorm, like the
    reference's DataParallel, config.py:114-118), announces them bucket by bucket in the schedule's order and
    must end with the mean of the two per-shard gradients in every parameter;
  * bench.py --gpus 2 starts two ranks by itself (launcher plumbing only, no GPU work)."""
import importlib
import json
import os
import socket
import subprocess
import sys

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    mod = importlib.import_module('single-image-super-resolution_amd.distributed')
    torch.manual_seed(0)
    params = [torch.nn.Parameter(torch.randn(s)) for s in [(7, 5), (3,), (64, 9), (1,)]]
    params.append(torch.nn.Parameter(torch.randn(4), requires_grad=False))
    for i, p in enumerate(params[:-1]):
        p.grad = torch.full_like(p, float(rank + 1) * (i + 1))
    red = mod.GradReducer(params, world, bucket_bytes=200, inplace_bytes=1000)     # several buckets, one in-place tensor
    red.all_reduce_mean()
    ok = all(torch.allclose(p.grad, torch.full_like(p, 1.5 * (i + 1))) for i, p in enumerate(params[:-1]))
    q.put((rank, ok, len(red.buckets)))
    dist.destroy_process_group()


def _run2(target, *extra):
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=target, args=(r, 2, port, q) + extra) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    return res


def test_grad_reducer_world2_gloo():
    res = _run2(_worker)
    assert all(ok for _, ok, _ in res), res
    assert res[0][2] >= 2


def _strided_worker(rank, world, port, q):
    """gradients that are transposed views (what ``x.t().contiguous().t()`` or a matmul backward may hand over): the exchange
    packs them into its flat message and must write the mean back THROUGH their strides"""
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    mod = importlib.import_module('single-image-super-resolution_amd.distributed')

    def grads_for(r):
        g = torch.Generator().manual_seed(100 + r)
        return [torch.randn(5, 7, generator=g).t(),                  # (7, 5) with strides (1, 7)
                torch.randn(3, generator=g),
                torch.randn(4, 6, generator=g),
                torch.randn(2, 3, 4, generator=g).permute(2, 0, 1)]   # (4, 2, 3) with strides (1, 12, 4)

    every = [grads_for(r) for r in range(world)]
    want = [sum(gs[i] for gs in every) / world for i in range(4)]
    bad = []
    # alone (a bucket of one non-contiguous gradient), then mixed with contiguous small ones in one flat message
    for name, idx in (('alone', [0]), ('mixed', [0, 1, 2, 3])):
        params = [torch.nn.Parameter(torch.zeros(tuple(every[rank][i].shape))) for i in idx]
        for p, i in zip(params, idx):
            p.grad = grads_for(rank)[i]
        strides = [p.grad.stride() for p in params]
        if params[0].grad.is_contiguous():
            bad.append((name, 0, 'the test gradient is contiguous'))
        red = mod.GradReducer(params, world)
        if len(red.buckets) != 1:
            bad.append((name, 'buckets', len(red.buckets)))
        red.all_reduce_mean()
        for p, i, st in zip(params, idx, strides):
            if p.grad.stride() != st:
                bad.append((name, i, 'strides', p.grad.stride(), st))
            err = float((p.grad - want[i]).abs().max())
            if not err <= 1e-6:
                bad.append((name, i, 'value', err))
    q.put((rank, bad))
    dist.destroy_process_group()


def test_grad_reducer_non_contiguous_gradients_get_the_mean():
    res = _run2(_strided_worker)
    assert len(res) == 2
    for rank, bad in res:
        assert not bad, (rank, bad)


def _bucket_worker(rank, world, port, q):
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    sys.path.insert(0, ROOT)
    from helpers import load_case, oracle_fwd_bwd                      # the CPU oracle: checker only
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    mod = importlib.import_module('single-image-super-resolution_amd.distributed')
    mg = importlib.import_module('single-image-super-resolution_amd.model_generator')
    z, cfg, state, _, _ = load_case('gen_x2_nosn_w16')                 # B = 2: one patch per rank
    x, r = torch.from_numpy(z['x']), torch.from_numpy(z['r'])
    shard = [oracle_fwd_bwd(cfg, state, x[k:k + 1], r[k:k + 1])[2] for k in range(world)]     # both shards' gradients
    want = {k: sum(s[k] for s in shard) / world for k in shard[0]}
    net = mg.Generator(cfg['n_blocks'], cfg['nf'], cfg['nl'], cfg['list_scales'], use_sn=cfg['use_sn'])
    net.load_state_dict(state, strict=True)
    red = mod.GradReducer(net, world)                                  # attaches itself as the module's gradient sink
    assert net._sisr_grad_sink is red
    named = dict(net.named_parameters())
    mine = {k: shard[rank][k].clone() for k in named}
    # the schedule's announcement order (generator_engine.run_backward): output/upscale/trunk-end, blocks, first conv
    order = [[k for k in named if k.startswith(('end.', 'upscale.', 'block_list_end.'))],
             [k for k in named if k.startswith('block_list.')],
             [k for k in named if k.startswith('first_layers.')]]
    assert sorted(sum(order, [])) == sorted(named)
    for tag, keys in zip(('tail', 'blocks4', mod.FINAL), order):
        red.ready([(named[k], mine[k]) for k in keys], tag)
    red.backward_end()
    for k, p in named.items():
        p.grad = mine[k]                                               # what autograd's AccumulateGrad does next
    red.finish()                                                       # nothing left to reduce: all were announced
    err = max(float((named[k].grad - want[k]).abs().max()) / max(float(want[k].abs().max()), 1e-12) for k in named)
    q.put((rank, err, dict(red.stats)))
    dist.destroy_process_group()


def test_bucket_ready_interface_gives_the_mean_of_the_per_shard_oracle_gradients():
    res = _run2(_bucket_worker)
    for rank, err, stats in res:
        assert err < 1e-6, (rank, err)
        assert stats == {'early_buckets': 3, 'late_buckets': 0}, stats


def _dis_bucket_worker(rank, world, port, q):
    """the discriminator's schedule (discriminator_engine.run_backward): TWO backward passes per sweep (real batch and fake
    batch, train.py:132,156), each announcing fc first, then the conv layers deepest first; every pass is reduced where it lies
    and autograd's sum of the reduced passes must be the mean over ranks of the summed per-shard oracle gradients"""
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    sys.path.insert(0, ROOT)
    from helpers import load_case, oracle_fwd_bwd                      # the CPU oracle: checker only
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    mod = importlib.import_module('single-image-super-resolution_amd.distributed')
    md = importlib.import_module('single-image-super-resolution_amd.model_discriminator')
    z, cfg, state, _, _ = load_case('dis_16px_w16')
    x, r = torch.from_numpy(z['x']), torch.from_numpy(z['r'])
    nb = x.shape[0] // world
    # per rank: a "real" pass on its shard and a "fake" pass on the flipped shard
    def passes(k):
        xs, rs = x[k * nb:(k + 1) * nb], r[k * nb:(k + 1) * nb]
        return [oracle_fwd_bwd(cfg, state, xs, rs)[2], oracle_fwd_bwd(cfg, state, xs.flip(-1), rs)[2]]
    shard = [passes(k) for k in range(world)]
    want = {k: sum(s[0][k] + s[1][k] for s in shard) / world for k in shard[0][0]}
    net = md.Discriminator(tuple(cfg['input_shape']), cfg['list_n_features'], cfg['list_stride'])
    net.load_state_dict(state, strict=True)
    red = mod.GradReducer(net, world, name='D:', inplace_bytes=1 << 12)     # fc.0.weight travels in place, the rest as one flat message
    assert net._sisr_grad_sink is red
    named = dict(net.named_parameters())
    n_blocks = len(cfg['list_n_features']) - 1
    de = importlib.import_module('single-image-super-resolution_amd.discriminator_engine')
    # the schedule's buckets: head, then conv blocks from the deepest in groups of SINK_CONVS, then whatever is left + conv.0
    order, tags, done = [[k for k in named if k.startswith('fc.')]], ['fc'], 0
    blocks = list(range(n_blocks - 1, -1, -1))
    cur = []
    for i in blocks:
        cur += [k for k in named if k.startswith('conv.2.%d.' % i)]
        done += 1
        if done % de.SINK_CONVS == 0 and i > 0:
            order.append(cur); tags.append('convs%d' % done); cur = []
    order.append(cur + [k for k in named if k.startswith('conv.0.')]); tags.append(mod.FINAL)
    assert sorted(sum(order, [])) == sorted(named)
    total = {k: torch.zeros_like(v) for k, v in named.items()}
    for pss in shard[rank]:
        mine = {k: pss[k].clone() for k in named}
        for tag, keys in zip(tags, order):
            red.ready([(named[k], mine[k]) for k in keys], tag)
        red.backward_end()
        for k in named:
            total[k] += mine[k]                                        # autograd adds the (already reduced) passes
    for k, p in named.items():
        p.grad = total[k]
    red.finish()                                                       # nothing left: every pass announced everything
    # a muted reducer (the G step's pass through D) must not touch anything
    red.enabled = False
    before = {k: p.grad.clone() for k, p in named.items()}
    red.ready([(named[k], named[k].grad) for k in named], 'fc')
    red.backward_end()
    red.enabled = True
    same = all(torch.equal(before[k], named[k].grad) for k in named)
    err = max(float((named[k].grad - want[k]).abs().max()) / max(float(want[k].abs().max()), 1e-12) for k in named)
    q.put((rank, err, dict(red.stats), same, len(tags)))
    dist.destroy_process_group()


def test_discriminator_bucket_ready_schedule_two_passes_per_sweep():
    res = _run2(_dis_bucket_worker)
    for rank, err, stats, same, n_tags in res:
        assert err < 1e-6, (rank, err)
        assert same
        assert stats['late_buckets'] == 0 and stats['early_buckets'] == 2 * n_tags and stats['early_buckets'] >= 3, stats


def _gather_worker(rank, world, port, q):
    """GradReducer.gather: the factors of a rank-B product travel instead of the product; every rank forms the mean itself"""
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    mod = importlib.import_module('single-image-super-resolution_amd.distributed')
    g = torch.Generator().manual_seed(10 + rank)
    w = torch.nn.Parameter(torch.zeros(8, 12))
    small = torch.nn.Parameter(torch.zeros(5))
    red = mod.GradReducer([w, small], world)
    d1, x = torch.rand(4, 8, generator=g) - 0.5, torch.rand(4, 12, generator=g) - 0.5
    local = d1.t() @ x
    parts = [torch.empty_like(local) for _ in range(world)]
    dist.all_gather(parts, local)
    want = sum(parts) / world
    d1_all, x_all = torch.empty(world * 4, 8), torch.empty(world * 4, 12)
    assert red.gather([(d1, d1_all), (x, x_all)], 'fc1_factors', done=[w])
    red.wait()
    got = d1_all.t() @ x_all / world
    # the post-backward pass must leave the factored parameter alone and still reduce the other one
    w.grad, small.grad = got.clone(), torch.full((5,), float(rank))
    red.finish()
    ok = torch.equal(w.grad, got) and float((small.grad - (world - 1) / 2.0).abs().max()) < 1e-6
    muted = mod.GradReducer([w], world)
    muted.enabled = False
    q.put((rank, float((got - want).abs().max()), ok, dict(red.stats), muted.gather([(d1, d1_all)], 'x')))
    dist.destroy_process_group()


def test_factors_of_a_gradient_travel_by_all_gather_world2():
    res = _run2(_gather_worker)
    for rank, err, ok, stats, muted in res:
        assert err < 1e-6 and ok and muted is False, (rank, err, ok, muted)
        assert stats == {'early_buckets': 1, 'late_buckets': 1}, stats


def test_bench_gpus_2_starts_two_ranks_itself():
    """`python bench.py --gpus 2` with no launcher environment must start two rank processes before any GPU call
    (here: the launcher self-test, which all-reduces a 1 over the ranks on gloo and prints the count)"""
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--backend', 'gloo', '--dry-run-ranks'],
                       capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith('{')][-1]
    rec = json.loads(line)
    assert rec == {'dry_run': True, 'n_gpus': 2, 'world': 2}
    # a launcher world size that contradicts --gpus is refused
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '3', '--dry-run-ranks'],
                       capture_output=True, text=True, env=dict(env, WORLD_SIZE='2', RANK='0'), timeout=120, cwd=ROOT)
    assert r.returncode == 2 and 'WORLD_SIZE=2' in r.stderr
