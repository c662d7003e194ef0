"""GPU: optim.Adam(capturable=True) -- step counts, learning rate, global-norm clipping and skip-on-non-finite on the device
 -- against the host-state fused Adam and torch.optim.Adam, through state dicts, and replayed from HIP
graphs up to a whole SRGAN iteration (G forward, D step + Adam, G step + Adam) as ONE graph.

The tensor set is awkward on purpose: numel 1 / 35 / 1027 (scalar path, tails), 4096 / 4097 (exactly one chunk of the block
mapping; one chunk plus one element), (64,64,3,3) (nine full chunks, 16-byte path), (5,7), and 300 tensors of numel 3 (more
tensors than one workgroup of the prepare launch has threads).

Tolerances: 1e-6 relative per tensor is test_gpu_optim.py's bound for the same fp32 formula (only the double pow moved to the
device).  With clipping the moments get 2e-6: that 1e-6 plus one fp32 rounding of the clip coefficient (6e-8), which enters
exp_avg_sq twice.  The norm itself is accumulated in double, so only its final fp32 rounding separates it from an fp64 norm."""
import copy

import pytest
import torch

from gpu_helpers import OffsetViews, maxrel, pkg

pytestmark = pytest.mark.gpu
TOL = 1e-6
SHAPES = [(1,), (35,), (1027,), (4096,), (4097,), (64, 64, 3, 3), (5, 7)] + [(3,)] * 300
I1027, ICONV = 2, 5


def _params(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter((torch.rand(s, generator=g) - 0.5).cuda()) for s in SHAPES]


def _grads(gen, scale=1.0):
    return [((torch.rand(s, generator=gen) - 0.5) * scale).cuda() for s in SHAPES]


def _set_grads(params, grads):
    for p, g in zip(params, grads):
        p.grad = None if g is None else g.clone()


def _assert_same_state(oa, pa, ob, pb, tol_p=TOL, tol_m=TOL):
    for k, (p, q) in enumerate(zip(pa, pb)):
        assert maxrel(p, q) < tol_p, k
        assert maxrel(oa.state[p]['exp_avg'], ob.state[q]['exp_avg']) < tol_m, k
        assert maxrel(oa.state[p]['exp_avg_sq'], ob.state[q]['exp_avg_sq']) < tol_m, k


@pytest.mark.parametrize('wd', [0.0, 0.01])
def test_capturable_adam_matches_the_host_state_fused_adam(wd):
    """6 steps under LambdaLR with a float lr on one twin and a tensor lr on the other; at step 3 one parameter has no gradient"""
    op = pkg('optim')
    pf, pt, pr = _params(1), _params(1), _params(1)
    base_lr, f = 1e-3, 0.1 ** (1 / 50)
    of = op.Adam(pf, lr=base_lr, weight_decay=wd, capturable=True)
    ot = op.Adam(pt, lr=torch.tensor(base_lr, device='cuda'), weight_decay=wd, capturable=True)
    ref = op.Adam(pr, lr=base_lr, weight_decay=wd)
    scheds = [torch.optim.lr_scheduler.LambdaLR(o, lr_lambda=lambda it: f ** it) for o in (of, ot, ref)]
    lr_tensor = ot.param_groups[0]['lr']
    gen = torch.Generator().manual_seed(7)
    for it in range(6):
        grads = _grads(gen, 10.0 ** ((it % 3) - 1))
        if it == 3:
            grads[ICONV] = None
        for ps in (pf, pt, pr):
            _set_grads(ps, grads)
        for o in (of, ot, ref):
            o.step()
        for s in scheds:
            s.step()
    assert ot.param_groups[0]['lr'] is lr_tensor                    # the scheduler filled the tensor the kernels read
    for o, ps in ((of, pf), (ot, pt)):
        _assert_same_state(o, ps, ref, pr)
        for p, q in zip(ps, pr):
            step = o.state[p]['step']
            assert step.is_cuda and step.dim() == 0 and step.dtype == torch.float32
            assert float(step) == float(ref.state[q]['step'])
    assert float(of.state[pf[ICONV]]['step']) == 5.0 and float(of.state[pf[0]]['step']) == 6.0


def _other(kind, params, lr):
    if kind == 'torch':
        return torch.optim.Adam(params, lr=lr)
    if kind == 'torch_capturable':
        return torch.optim.Adam(params, lr=lr, capturable=True)
    return pkg('optim').Adam(params, lr=lr)


def _ptrs(opt, params):
    return [(opt.state[p]['exp_avg'].data_ptr(), opt.state[p]['exp_avg_sq'].data_ptr(), opt.state[p]['step'].data_ptr())
            for p in params]


@pytest.mark.parametrize('kind', ['torch', 'torch_capturable', 'fused'])
def test_state_dicts_travel_both_ways_and_never_move_the_state(kind):
    op = pkg('optim')
    gen = torch.Generator().manual_seed(11)
    g1, g2, g3 = _grads(gen), _grads(gen), _grads(gen)
    # ---- other -> capturable: a donor with two steps of history is loaded over an optimizer that has one
    pa, pb = _params(2), _params(3)
    oa, ob = op.Adam(pa, lr=1e-3, capturable=True), _other(kind, pb, 1e-3)
    _set_grads(pa, g3); oa.step()
    for g in (g1, g2):
        _set_grads(pb, g); ob.step()
    before = _ptrs(oa, pa)
    oa.load_state_dict(copy.deepcopy(ob.state_dict()))
    assert _ptrs(oa, pa) == before
    with torch.no_grad():
        for p, q in zip(pa, pb):
            p.copy_(q)
    _set_grads(pa, g3); _set_grads(pb, g3)
    oa.step(); ob.step()
    _assert_same_state(oa, pa, ob, pb)
    assert _ptrs(oa, pa) == before
    assert all(float(oa.state[p]['step']) == 3.0 for p in pa)
    # ---- capturable -> other: the three steps of history above go into a fresh optimizer
    pc = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    oc = _other(kind, pc, 1e-3)
    oc.load_state_dict(copy.deepcopy(oa.state_dict()))
    _set_grads(pa, g1); _set_grads(pc, g1)
    oa.step(); oc.step()
    _assert_same_state(oa, pa, oc, pc)
    assert all(float(oc.state[q]['step']) == 4.0 for q in pc)
    # ---- zero_state: in place
    oa.zero_state()
    assert _ptrs(oa, pa) == before
    for p in pa:
        st = oa.state[p]
        assert float(st['step']) == 0.0 and not bool(st['exp_avg'].any()) and not bool(st['exp_avg_sq'].any())
    fresh = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    of = op.Adam(fresh, lr=1e-3, capturable=True)
    _set_grads(pa, g2); _set_grads(fresh, g2)
    oa.step(); of.step()
    assert all(torch.equal(p, q) for p, q in zip(pa, fresh))


def _norm64(grads):
    return float(torch.sqrt(sum((g.double() ** 2).sum() for g in grads)))


@pytest.mark.parametrize('factor', [0.5, 2.0], ids=['max_below_norm', 'max_above_norm'])
def test_global_norm_and_clipping_match_torch_adam_on_fp64_scaled_gradients(factor):
    op = pkg('optim')
    gen = torch.Generator().manual_seed(13)
    steps = [_grads(gen), _grads(gen, 3.0)]
    max_norm = factor * _norm64(steps[0])
    pa, pb = _params(4), _params(4)
    oa, ob = op.Adam(pa, lr=1e-3, weight_decay=0.01, max_grad_norm=max_norm), torch.optim.Adam(pb, lr=1e-3, weight_decay=0.01)
    for grads in steps:
        norm = _norm64(grads)
        coef = min(1.0, max_norm / (norm + 1e-6))
        assert (coef < 1.0) == (factor < 1.0 or grads is steps[1])
        _set_grads(pa, grads)
        _set_grads(pb, [(g.double() * coef).float() for g in grads])
        kept = [p.grad.clone() for p in pa]
        oa.step(); ob.step()
        got = oa.grad_norm
        assert got.is_cuda and got.dim() == 0
        assert abs(float(got) - norm) <= 1e-6 * norm
        assert all(torch.equal(p.grad, k) for p, k in zip(pa, kept))           # the gradients are only read
    _assert_same_state(oa, pa, ob, pb, tol_p=1e-6, tol_m=2e-6)
    first = oa.grad_norm.clone()
    oa.step()                                                                   # same gradients again: the same bits
    assert torch.equal(oa.grad_norm, first)
    assert int(oa.skipped_steps) == 0


def test_capturable_adam_on_offset_views_matches_torch_adam_and_keeps_their_neighbours():
    """parameters and a gradient that are only 4-byte aligned (gpu_helpers.OffsetViews) take the 4-byte path of the step kernel"""
    a, b = OffsetViews(6), OffsetViews(6)
    oa, ob = pkg('optim').Adam(a.params, lr=1e-3, weight_decay=0.01, capturable=True), torch.optim.Adam(b.params, lr=1e-3, weight_decay=0.01)
    ga, gb = torch.Generator().manual_seed(8), torch.Generator().manual_seed(8)
    for it in range(3):
        a.set_grads(ga, 10.0 ** (it - 1)); b.set_grads(gb, 10.0 ** (it - 1))
        oa.step(); ob.step()
    _assert_same_state(oa, a.params, ob, b.params)
    assert a.edges_intact()


def test_clipped_adam_on_offset_views_matches_torch_adam_on_fp64_scaled_gradients():
    """max_grad_norm=1.0: the sum-of-squares kernel reads the offset gradient (and the gradients of the offset parameters) too; the
    comparison and the bounds of test_global_norm_and_clipping_match_torch_adam_on_fp64_scaled_gradients"""
    a, b = OffsetViews(6), OffsetViews(6)
    oa, ob = pkg('optim').Adam(a.params, lr=1e-3, weight_decay=0.01, max_grad_norm=1.0), torch.optim.Adam(b.params, lr=1e-3, weight_decay=0.01)
    ga, gb = torch.Generator().manual_seed(8), torch.Generator().manual_seed(8)
    for it in range(3):
        a.set_grads(ga, 10.0 ** (it - 1)); b.set_grads(gb, 10.0 ** (it - 1))
        norm = _norm64([p.grad for p in a.params])
        coef = min(1.0, 1.0 / (norm + 1e-6))
        assert coef < 1.0
        for q in b.params:
            q.grad = (q.grad.double() * coef).float()
        kept = a.grad_view.clone()
        oa.step(); ob.step()
        assert abs(float(oa.grad_norm) - norm) <= 1e-6 * norm
        assert torch.equal(a.grad_view, kept)                                   # the gradients are only read
    _assert_same_state(oa, a.params, ob, b.params, tol_p=1e-6, tol_m=2e-6)
    assert a.edges_intact()
    assert int(oa.skipped_steps) == 0


def _snapshot(opt, params):
    return [(p.detach().clone(), opt.state[p]['exp_avg'].clone(), opt.state[p]['exp_avg_sq'].clone(), opt.state[p]['step'].clone())
            for p in params]


@pytest.mark.parametrize('case', ['inf_last_of_1027', 'nan_middle_of_conv'])
def test_a_non_finite_gradient_skips_the_whole_step(case):
    op = pkg('optim')
    gen = torch.Generator().manual_seed(17)
    g1, bad, g2 = _grads(gen), _grads(gen), _grads(gen)
    if case == 'inf_last_of_1027':
        bad[I1027][-1] = float('inf')
    else:
        bad[ICONV].view(-1)[bad[ICONV].numel() // 2] = float('nan')
    pa, pb = _params(5), _params(5)
    oa, ob = op.Adam(pa, lr=1e-3, weight_decay=0.01, skip_nonfinite=True), op.Adam(pb, lr=1e-3, weight_decay=0.01, skip_nonfinite=True)
    _set_grads(pa, g1); _set_grads(pb, g1)
    oa.step(); ob.step()
    before = _snapshot(oa, pa)
    _set_grads(pa, bad)
    oa.step()
    for old, new in zip(before, _snapshot(oa, pa)):
        assert all(torch.equal(a, b) for a, b in zip(old, new))
    assert int(oa.skipped_steps) == 1 and not bool(torch.isfinite(oa.grad_norm))
    _set_grads(pa, g2); _set_grads(pb, g2)
    oa.step(); ob.step()                                                        # the twin never saw the bad step
    for a, b in zip(_snapshot(oa, pa), _snapshot(ob, pb)):
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert int(oa.skipped_steps) == 1 and int(ob.skipped_steps) == 0
    assert bool(torch.isfinite(oa.grad_norm)) and float(oa.state[pa[0]]['step']) == 2.0


def test_gradients_of_magnitude_1e20_are_not_skipped():
    """an fp32 square overflows at |g| ~ 1.8e19; the norm is squared and summed in double"""
    op = pkg('optim')
    pa = _params(6)
    oa = op.Adam(pa, lr=1e-3, max_grad_norm=1.0, skip_nonfinite=True)
    grads = [torch.full(s, 1e20).cuda() for s in SHAPES]
    _set_grads(pa, grads)
    before = [p.detach().clone() for p in pa]
    oa.step()
    norm = _norm64(grads)
    assert int(oa.skipped_steps) == 0 and bool(torch.isfinite(oa.grad_norm))
    assert abs(float(oa.grad_norm) - norm) <= 1e-6 * norm
    assert all(float(oa.state[p]['step']) == 1.0 for p in pa)
    assert all(bool(torch.isfinite(p).all()) and not torch.equal(p, b) for p, b in zip(pa, before))


def _replay_setup(seed, **adam_kw):
    params = _params(seed)
    scale = torch.ones((), device='cuda')             # static input: rewritten in place before every run

    def run(opt):
        for p in params:
            p.grad = None
        loss = sum((p * p).sum() for p in params) * scale
        loss.backward()
        opt.step()
        return loss
    return params, scale, run


SCALES = [1.0, 0.5, 2.0, 1.5, 0.25, 3.0, 0.75]


def _replayed(lr):
    G, op = pkg('graph'), pkg('optim')
    f = 0.1 ** (1 / 10)
    params, scale, run = _replay_setup(8)
    opt = op.Adam(params, lr=lr, capturable=True)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lambda it: f ** it)
    fed = iter(SCALES)

    def fn():
        return run(opt)
    # the two warm-up runs are real steps at lr0 (both read the first scale); the capture itself executes nothing
    scale.fill_(next(fed))
    step = G.GraphedStep(fn, warmup=2)
    assert len(step.graphs) == 1 and step.captures_optimizer
    next(fed)
    for _ in range(5):
        scale.fill_(next(fed))
        step()
        sched.step()
    return opt, params


def _eager_twin():
    op = pkg('optim')
    f = 0.1 ** (1 / 10)
    params, scale, run = _replay_setup(8)
    opt = op.Adam(params, lr=1e-3)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lambda it: f ** it)
    for k, s in enumerate(SCALES):
        scale.fill_(SCALES[0] if k < 2 else s)
        run(opt)
        if k >= 2:
            sched.step()
    return opt, params


def test_replayed_step_follows_a_tensor_lr_and_a_baked_float_lr_does_not():
    ref, pr = _eager_twin()
    opt, params = _replayed(torch.tensor(1e-3, device='cuda'))
    for k, (p, q) in enumerate(zip(params, pr)):
        assert maxrel(p, q) < TOL, k
    assert all(float(opt.state[p]['step']) == 7.0 for p in params)
    # a float lr is mirrored by EAGER steps only: the replays keep lr0, and the comparison above sees it
    opt, params = _replayed(1e-3)
    assert all(float(opt.state[p]['step']) == 7.0 for p in params)
    assert max(maxrel(p, q) for p, q in zip(params, pr)) > 100 * TOL


def test_replays_with_a_captured_step_invalidate_the_weight_caches_and_others_do_not():
    E, G, op = pkg('engine'), pkg('graph'), pkg('optim')
    params, scale, run = _replay_setup(9)
    opt = op.Adam(params, lr=torch.tensor(1e-3, device='cuda'), capturable=True)
    with_step = G.GraphedStep(lambda: run(opt))
    x = torch.ones(8, device='cuda')
    without = G.GraphedStep(lambda: x * 2)
    assert with_step.captures_optimizer and not without.captures_optimizer
    epoch = E._WEIGHT_EPOCH[0]
    without()
    assert E._WEIGHT_EPOCH[0] == epoch
    with_step()
    assert E._WEIGHT_EPOCH[0] == epoch + 1
    with_step()
    assert E._WEIGHT_EPOCH[0] == epoch + 2


def test_first_step_inside_a_capture_is_refused_with_a_reason():
    G, op = pkg('graph'), pkg('optim')
    params, scale, run = _replay_setup(10)
    opt = op.Adam(params, lr=1e-3, capturable=True)
    _set_grads(params, _grads(torch.Generator().manual_seed(3)))
    with pytest.raises(G.GraphCaptureError, match='warm-up'):
        G.GraphedStep(opt.step, warmup=0)              # nothing allocated yet, and a captured step needs final addresses
    run(opt)                                           # the process is still usable, and so is the optimizer
    assert float(opt.state[params[0]]['step']) == 1.0


def _snapshot_net(net):
    return {k: v.clone() for k, v in net.state_dict().items()}


@pytest.mark.parametrize('build', ['fp32', 'bf16'])
def test_one_graph_srgan_iteration_with_both_adam_steps_inside(build):
    """test_gpu_configs.py's cfg2 iteration with one generator forward, shrunk, with od.step() and og.step() INSIDE the captured
    function and no segment boundary: one graph whose replays give the losses and parameters of the eager iterations"""
    E, G = pkg('engine'), pkg('graph')
    mg, md, mce, ut, op = (pkg('model_generator'), pkg('model_discriminator'), pkg('model_content_extractor'),
                           pkg('utils'), pkg('optim'))
    B = 2
    E.set_precision(build)
    try:
        dev = torch.device('cuda')
        hr = (torch.rand((B, 3, 16, 16), generator=torch.Generator().manual_seed(51)) * 2 - 1).cuda()

        def setup():
            torch.manual_seed(0)
            net_g = mg.Generator(2, 16, 64, [2], use_sn=True).to(dev).train()
            net_d = md.Discriminator((3, 16, 16), [16, 16, 32, 32], [1, 2, 1, 2]).to(dev).train()
            ext = mce.identity()
            og = op.Adam(net_g.parameters(), lr=1e-5, capturable=True)
            od = op.Adam(net_d.parameters(), lr=1e-5, capturable=True)
            crit = torch.nn.BCELoss()
            ones, red, zeros = torch.ones(B, device=dev), torch.full((B,), .9, device=dev), torch.zeros(B, device=dev)

            def both():
                lr = ut.lr_from_hr(hr, (8, 8), device=dev)
                fake = net_g(lr)
                net_d.zero_grad()
                err_d = crit(net_d(hr).view(-1), red) + crit(net_d(fake.detach()).view(-1), zeros)
                err_d.backward()
                od.step()
                net_g.zero_grad()
                err_g = crit(net_d(fake).view(-1), ones) * 5e-2 + torch.mean(torch.pow(ext(hr) - ext(fake), 2))
                err_g.backward()
                og.step()
                return err_d, err_g
            return net_g, net_d, og, od, both
        net_g, net_d, og, od, both = setup()
        ref_losses = []
        for _ in range(3):
            ed, eg = both()
            ref_losses.append((float(ed), float(eg)))
        g1, d1 = _snapshot_net(net_g), _snapshot_net(net_d)
        assert all(0 < a < 100 and 0 < b < 100 for a, b in ref_losses)

        net_g, net_d, og, od, both = setup()
        state_g, state_d = _snapshot_net(net_g), _snapshot_net(net_d)
        step = G.GraphedStep(both)
        assert len(step.graphs) == 1 and step.captures_optimizer
        net_g.load_state_dict(state_g); net_d.load_state_dict(state_d)          # the warm-ups advanced SN / BN / Adam state
        og.zero_state(); od.zero_state()                                          # (state.clear() would orphan the capture)

        def d_eval(net):
            net.eval()
            with torch.no_grad():
                out = net(hr).clone()
            net.train()
            return out
        d_eval(net_d)                                                            # an eager forward BEFORE the replays packs weights
        losses = []
        for _ in range(3):
            ed, eg = step()
            losses.append((float(ed), float(eg)))
        # an eager forward right after the replays must see the replayed parameters, not an image packed before them
        after = d_eval(net_d)
        fresh = md.Discriminator((3, 16, 16), [16, 16, 32, 32], [1, 2, 1, 2]).to(dev)
        fresh.load_state_dict(net_d.state_dict())
        assert torch.equal(after, d_eval(fresh))
        for (a, b), (c, d) in zip(losses, ref_losses):
            assert abs(a - c) <= 1e-6 * max(1.0, abs(c)) and abs(b - d) <= 1e-6 * max(1.0, abs(d)), (losses, ref_losses)
        gs, ds = _snapshot_net(net_g), _snapshot_net(net_d)
        for k in g1:
            if g1[k].is_floating_point():
                assert float((gs[k] - g1[k]).abs().max()) <= 1e-6 * max(1.0, float(g1[k].abs().max())), k
        for k in d1:
            if d1[k].is_floating_point():
                assert float((ds[k] - d1[k]).abs().max()) <= 1e-6 * max(1.0, float(d1[k].abs().max())), k
        assert float(od.state[next(iter(net_d.parameters()))]['step']) == 3.0
    finally:
        E.set_precision('fp32')
