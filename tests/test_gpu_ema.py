"""GPU: ema.WeightEMA (csrc/optim.hip: ema_prepare / ema_update / ema_swap) -- the averaged values against
the recursion in float64 on the CPU, bit-level guarantees (unchanged parameters, copied buffers, swap and swap back), replay
from a HIP graph behind a capturable Adam step, following that optimizer's skipped steps, checkpoints, and
metrics.evaluate_generator(ema=...).

The toy module holds test_gpu_adam_capturable.py's awkward tensor set: numel 1 / 35 / 1027 (scalar path, tails), 4096 / 4097
(exactly one chunk of the block mapping; one chunk plus one element), (64,64,3,3) (nine full chunks, 16-byte path), (5,7), 300
tensors of numel 3, plus a 1024-element parameter that is a view ONE element into its storage (numel % 4 == 0 but only 4-byte
aligned: the 16-byte path must not take it), an fp32 buffer (copied by the launch) and an int64 buffer (copied by torch).

Value bound: 4 k 2^-24 M absolute after k updates, M = the largest magnitude among the parameters and the initial shadows: per
update one rounding each for p - e, the product and the sum, plus the fp32 rounding of 1 - d; earlier errors contract by d."""
import copy

import pytest
import torch

from gpu_helpers import pkg

pytestmark = pytest.mark.gpu
SHAPES = [(1,), (35,), (1027,), (4096,), (4097,), (64, 64, 3, 3), (5, 7)] + [(3,)] * 300
I1027, ICONV = 2, 5
K = 8


class Toy(torch.nn.Module):
    """built on the device: .cuda() would re-allocate the offset view compactly"""

    def __init__(self, seed):
        super().__init__()
        g = torch.Generator(device='cuda').manual_seed(seed)
        rand = lambda *s: torch.rand(*s, generator=g, device='cuda') - 0.5          # noqa: E731
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(rand(s)) for s in SHAPES])
        self.storage = rand(1028)
        self.odd = torch.nn.Parameter(self.storage[1:1025])
        self.register_buffer('stat', rand(67))
        self.register_buffer('ticks', torch.tensor(3, dtype=torch.int64, device='cuda'))
        assert self.odd.data_ptr() % 16 == 4 and self.odd.is_contiguous()


def _shadows(ema):
    return ema.state_dict()['shadow']


def _bits(t):
    return t.detach().contiguous().view(torch.int32) if t.dtype == torch.float32 else t.detach()


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _snapshot(tensors):
    return {k: v.detach().clone() for k, v in tensors.items()}


def _flat64(tensors):
    return torch.cat([t.detach().reshape(-1) for t in tensors]).double().cpu()


def _randomise(toy, gen, scale=1.0, skip=()):
    with torch.no_grad():
        for k, p in toy.named_parameters():
            if k not in skip:
                p.copy_((torch.rand(p.shape, generator=gen, device='cuda') - 0.5) * scale)
        toy.stat.copy_(torch.rand(toy.stat.shape, generator=gen, device='cuda'))
        toy.ticks += 1


@pytest.mark.parametrize('warmup', [10, None], ids=['warmup10', 'constant'])
def test_averages_match_the_fp64_recursion_and_buffers_are_copied(warmup):
    toy = Toy(1)
    ema = pkg('ema').WeightEMA(toy, decay=0.999, warmup=warmup)
    names = [k for k, _ in toy.named_parameters()]
    assert len(names) == len(SHAPES) + 1
    shadows = _shadows(ema)
    assert list(shadows) == names + ['stat', 'ticks']
    ref = _flat64([shadows[k] for k in names])
    assert torch.equal(ref, _flat64(toy.parameters()))                   # shadows start as copies
    big = float(ref.abs().max())
    gen = torch.Generator(device='cuda').manual_seed(2)
    for n in range(K):
        _randomise(toy, gen, 10.0 ** ((n % 3) - 1))
        ema.update()
        p = _flat64(toy.parameters())
        big = max(big, float(p.abs().max()))
        ref = ref + (1.0 - ema.decay_at(n)) * (p - ref)
    got = _flat64([shadows[k] for k in names])
    err, bound = float((got - ref).abs().max()), 4 * K * 2.0 ** -24 * big
    print('warmup %s: max abs error %.3e, bound %.3e (M = %.3f)' % (warmup, err, bound, big))
    assert err <= bound
    assert float((got - _flat64(toy.parameters())).abs().max()) > 1e-3   # ... and is an average, not the last value
    assert _same_bits(shadows['stat'], toy.stat) and torch.equal(shadows['ticks'], toy.ticks) and int(toy.ticks) == 3 + K
    n_upd = ema.num_updates
    assert n_upd.is_cuda and n_upd.dim() == 0 and n_upd.dtype == torch.int32 and int(n_upd) == K


def test_frozen_and_unchanged_parameters_keep_their_shadow_bits():
    toy = Toy(3)
    frozen = ['ps.%d' % ICONV, 'ps.%d' % I1027, 'odd', 'ps.0']
    with torch.no_grad():
        toy.ps[ICONV].view(-1)[::7] = -0.0                              # e + omd * 0 would make these +0
        toy.ps[I1027][5] = -0.0
        toy.ps[I1027][6] = 1e-42                                          # a denormal
    for k in frozen[:2]:
        dict(toy.named_parameters())[k].requires_grad_(False)
    ema = pkg('ema').WeightEMA(toy, decay=0.9, warmup=2)
    first = _snapshot(_shadows(ema))
    ema.update()                                                          # nothing changed at all
    assert all(_same_bits(first[k], v) for k, v in _shadows(ema).items())
    gen = torch.Generator(device='cuda').manual_seed(4)
    for _ in range(3):
        _randomise(toy, gen, skip=frozen)
        ema.update()
    now = _shadows(ema)
    live = dict(toy.named_parameters())
    for k in frozen:
        assert _same_bits(first[k], now[k]) and _same_bits(now[k], live[k]), k
    assert not torch.equal(first['ps.3'], now['ps.3']) and int(ema.num_updates) == 4


def _live(module):
    return dict(module.state_dict(keep_vars=True))


def test_swap_exchanges_bits_in_place_and_applied_restores_on_an_exception():
    G = pkg('graph')
    toy = Toy(5)
    ema = pkg('ema').WeightEMA(toy, decay=0.5)
    _randomise(toy, torch.Generator(device='cuda').manual_seed(6))
    ema.update()
    with torch.no_grad():
        toy.ps[3][7] = float('nan')                                       # bits travel, whatever they mean
    live0, shadow0 = _snapshot(_live(toy)), _snapshot(_shadows(ema))
    assert set(live0) == set(shadow0) and not _same_bits(live0['ps.5'], shadow0['ps.5'])
    shadow0['ticks'] -= 2                                                 # make the int64 pair differ too
    _shadows(ema)['ticks'].copy_(shadow0['ticks'])
    ptrs = {k: v.data_ptr() for k, v in _live(toy).items()}, {k: v.data_ptr() for k, v in _shadows(ema).items()}
    E = pkg('engine')
    epoch = E._WEIGHT_EPOCH[0]
    ema.swap()
    assert E._WEIGHT_EPOCH[0] == epoch + 1
    assert all(_same_bits(v, shadow0[k]) for k, v in _live(toy).items())
    assert all(_same_bits(v, live0[k]) for k, v in _shadows(ema).items())
    ema.swap()
    assert all(_same_bits(v, live0[k]) for k, v in _live(toy).items())
    assert all(_same_bits(v, shadow0[k]) for k, v in _shadows(ema).items())
    with pytest.raises(KeyError, match='inside'):
        with ema.applied():
            assert all(_same_bits(v, shadow0[k]) for k, v in _live(toy).items())
            raise KeyError('inside')
    assert all(_same_bits(v, live0[k]) for k, v in _live(toy).items())
    assert all(_same_bits(v, shadow0[k]) for k, v in _shadows(ema).items())
    # a captured swap would change parameters on every replay with no host call: refused (the two warm-up runs cancel out)
    with pytest.raises(G.GraphCaptureError, match='swap'):
        G.GraphedStep(ema.swap)
    assert all(_same_bits(v, live0[k]) for k, v in _live(toy).items())
    assert all(_same_bits(v, shadow0[k]) for k, v in _shadows(ema).items())
    assert ptrs == ({k: v.data_ptr() for k, v in _live(toy).items()}, {k: v.data_ptr() for k, v in _shadows(ema).items()})
    ema.update()                                                          # the process and the average are still usable
    assert int(ema.num_updates) == 2


def test_a_moved_parameter_is_followed_eagerly_and_refused_inside_a_capture():
    G = pkg('graph')
    toy = Toy(7)
    ema = pkg('ema').WeightEMA(toy, decay=0.5)
    table = ema._table.data_ptr()
    with torch.no_grad():
        toy.ps[3].data = torch.full((4096,), 2.0, device='cuda')          # a new address
    before = _shadows(ema)['ps.3'].clone()
    ema.update()
    assert torch.equal(_shadows(ema)['ps.3'], before + 0.5 * (2.0 - before)) and ema._table.data_ptr() == table
    with torch.no_grad():
        toy.ps[3].data = torch.full((4096,), 3.0, device='cuda')
    with pytest.raises(G.GraphCaptureError, match='moved'):
        G.GraphedStep(ema.update, warmup=0)
    ema.update()
    assert int(ema.num_updates) == 2


SCALES = [1.0, 0.5, 2.0, 1.5, 0.25, 3.0, 0.75]


def _trainer(seed, **adam_kw):
    toy = Toy(seed)
    # (the optimizer steps the aligned tensors; the offset view is averaged all the same and must keep its bits)
    opt = pkg('optim').Adam(toy.ps.parameters(), lr=torch.tensor(1e-2, device='cuda'), capturable=True, **adam_kw)
    ema = pkg('ema').WeightEMA(toy, decay=0.9, warmup=3, follow=opt if adam_kw else None)
    scale = torch.ones((), device='cuda')                               # static input: rewritten in place before every run

    def run():
        for p in toy.parameters():
            p.grad = None
        loss = sum((p * p).sum() for p in toy.parameters()) * scale
        loss.backward()
        opt.step()
        ema.update()
        return loss
    return toy, opt, ema, scale, run


def test_update_replays_behind_a_captured_adam_step_bit_for_bit():
    G = pkg('graph')
    toy, opt, ema, scale, run = _trainer(8)
    fed = iter(SCALES)
    scale.fill_(next(fed))
    step = G.GraphedStep(run, warmup=2)                                  # two real runs on the first scale; the capture runs nothing
    assert len(step.graphs) == 1 and step.captures_optimizer
    next(fed)
    for _ in range(5):
        scale.fill_(next(fed))
        step()
    twin, _, ema2, scale2, run2 = _trainer(8)
    for k, s in enumerate(SCALES):
        scale2.fill_(SCALES[0] if k < 2 else s)
        run2()
    assert int(ema.num_updates) == int(ema2.num_updates) == 7
    a, b = _shadows(ema), _shadows(ema2)
    assert all(_same_bits(a[k], b[k]) for k in a)
    assert all(_same_bits(p, q) for p, q in zip(toy.parameters(), twin.parameters()))
    assert not torch.equal(a['ps.5'], dict(toy.named_parameters())['ps.5'])


def test_following_the_optimizer_a_skipped_step_leaves_shadows_and_count_alone():
    toy, opt, ema, scale, run = _trainer(9, skip_nonfinite=True)
    twin, opt2, ema2, scale2, run2 = _trainer(9, skip_nonfinite=True)
    run(); run2()
    before, count = _snapshot(_shadows(ema)), ema.num_updates.clone()
    scale.fill_(float('inf'))                                            # every gradient is infinite or NaN
    run()
    assert int(opt.skipped_steps) == 1 and int(opt.skip_flag) == 1
    now = _shadows(ema)
    assert all(_same_bits(before[k], now[k]) for k in before if k != 'ticks') and torch.equal(ema.num_updates, count)
    scale.fill_(0.5); scale2.fill_(0.5)
    run(); run2()                                                        # the twin never saw the bad step
    assert int(opt.skip_flag) == 0 and int(ema.num_updates) == int(ema2.num_updates) == 2
    a, b = _shadows(ema), _shadows(ema2)
    assert all(_same_bits(a[k], b[k]) for k in a)
    assert not _same_bits(a['ps.5'], before['ps.5'])


@pytest.mark.parametrize('kind', ['generator', 'suffix'])
def test_shadow_state_dict_loads_into_a_fresh_net_and_load_state_dict_keeps_addresses(kind):
    mg = pkg('model_generator')

    def make():
        net = mg.Generator(2, 16, 64, [2])
        return (mg.GeneratorSuffix(net) if kind == 'suffix' else net).cuda()
    torch.manual_seed(11)
    net = make()
    ema = pkg('ema').WeightEMA(net, decay=0.5, warmup=None)
    with torch.no_grad():
        for p in net.parameters():
            p.add_(torch.randn_like(p) * 0.05)
    ema.update()
    sd = ema.shadow_state_dict()
    assert list(sd.keys()) == list(net.state_dict().keys())
    live = net.state_dict()
    assert all(v.data_ptr() != live[k].data_ptr() for k, v in sd.items())
    assert any(not torch.equal(v, live[k]) for k, v in sd.items())
    fresh = make()
    fresh.load_state_dict(sd, strict=True)
    assert all(torch.equal(v, sd[k]) for k, v in fresh.state_dict().items())
    # state_dict -> load_state_dict of another average: values and count arrive, no shadow moves
    state = copy.deepcopy(ema.state_dict())
    assert set(state) == {'shadow', 'num_updates', 'decay', 'warmup'} and int(state['num_updates']) == 1
    other = pkg('ema').WeightEMA(fresh, decay=0.999, warmup=10)
    ptrs = [v.data_ptr() for v in _shadows(other).values()] + [other.num_updates.data_ptr()]
    other.load_state_dict(state)
    assert ptrs == [v.data_ptr() for v in _shadows(other).values()] + [other.num_updates.data_ptr()]
    assert all(_same_bits(v, state['shadow'][k]) for k, v in _shadows(other).items())
    assert int(other.num_updates) == 1 and other.decay == 0.5 and other.warmup is None
    del state['shadow'][next(iter(state['shadow']))]
    with pytest.raises(KeyError):
        other.load_state_dict(state)


def test_evaluate_generator_scores_the_averaged_weights_and_restores_the_live_ones():
    M, mg = pkg('metrics'), pkg('model_generator')
    torch.manual_seed(12)
    net = mg.Generator(2, 16, 64, [2]).cuda().train()
    hr = (torch.rand(4, 3, 32, 32, generator=torch.Generator().manual_seed(13)) * 2 - 1).cuda()
    ema = pkg('ema').WeightEMA(net, decay=0.5)
    with torch.no_grad():
        for p in net.parameters():
            p.add_(torch.randn_like(p) * 0.05)
        for k, b in net.named_buffers():
            if 'running' in k:
                b.add_(0.1)
    ema.update()
    with torch.no_grad():                                                # the live net moves on: shadows = neither old nor new weights
        for p in net.parameters():
            p.add_(torch.randn_like(p) * 0.05)
    twin = mg.Generator(2, 16, 64, [2]).cuda().train()
    twin.load_state_dict(ema.shadow_state_dict(), strict=True)
    before = _snapshot(_live(net))
    live_score = M.evaluate_generator(net, hr, (16, 16))                # an eager forward BEFORE the swap packs the live weights
    want, again = M.evaluate_generator(twin, hr, (16, 16)), M.evaluate_generator(twin, hr, (16, 16))
    assert all(torch.equal(want[k], again[k]) for k in want)           # the eval forward is a fixed schedule without atomics
    got = M.evaluate_generator(net, hr, (16, 16), ema=ema)
    print('psnr live %s ema %s twin %s' % (live_score['psnr'].tolist(), got['psnr'].tolist(), want['psnr'].tolist()))
    assert all(torch.equal(got[k], want[k]) for k in want)
    assert not torch.equal(got['psnr'], live_score['psnr']) and not torch.equal(got['ssim'], live_score['ssim'])
    assert net.training and all(_same_bits(v, before[k]) for k, v in _live(net).items())
    after = M.evaluate_generator(net, hr, (16, 16))                     # ... and the swap back is seen by the next forward
    assert all(torch.equal(after[k], live_score[k]) for k in after)
    with pytest.raises(ValueError):
        M.evaluate_generator(twin, hr, (16, 16), ema=ema)                # an average of another module
