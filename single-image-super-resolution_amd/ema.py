"""Exponential moving average (EMA) of a network's weights on the device: the copy a GAN trainer
evaluates and ships instead of the live weights, which oscillate from step to step.  The reference keeps none (ESRGAN-style
training is on its list of possible improvements, README.md).

``WeightEMA(module)`` holds a "shadow" of every tensor of ``module.state_dict()``:

* every parameter (walked through ``named_parameters()``, so a shared tensor is taken once; frozen ones included) is AVERAGED:
  ``e += (1 - d) * (p - e)`` with ``d = decay_at(n)`` for the n-th update;
* every fp32 buffer (BatchNorm running statistics, spectral-norm ``weight_u`` / ``weight_v``) is COPIED bit for bit by the same
  launch; a skipped update (``follow=``) skips them too;
* every other buffer (``num_batches_tracked``, int64) is copied by torch on the same stream -- on every update: these are
  counters, not weights.

``update()`` is two HIP launches on the current stream (``sisr_ema_prepare``, ``sisr_ema_update``: csrc/optim.hip) whatever the
number of tensors, reads nothing back and allocates nothing: shadows, update count, control block and descriptor table exist
from construction on, so it may be called inside a stream capture (graph.GraphedStep) right behind a capturable
``optim.Adam.step()`` without a warm-up of its own, and advances on every replay -- the update count and the decay schedule live
in device memory.  ``decay`` and ``warmup`` themselves are launch arguments: a captured update keeps those of its capture.

``swap()`` exchanges live and averaged tensors IN PLACE (no address moves: captured graphs and descriptor tables stay valid);
``applied()`` is the context manager around it; ``metrics.evaluate_generator(..., ema=ema)`` scores the averaged weights.

Limitation (the usual EMA-of-spectral-norm approximation): in eval mode the sigma that normalises an averaged ``weight_orig`` is
formed with the live ``u`` / ``v`` vectors, which are copied, not iterated against the averaged weight.

Data-parallel training needs nothing more: the ranks hold identical parameters after the all-reduced step, hence identical
averages.  Device fp32 contiguous parameters only, no fallback."""
import contextlib
import math
from collections import OrderedDict

import torch

from . import _lib as L
from . import engine as E


def _check_schedule(decay, warmup):
    decay = float(decay)
    if not 0.0 <= decay < 1.0:
        raise ValueError('WeightEMA: decay must be in [0, 1), got %r' % (decay,))
    if warmup is not None:
        warmup = float(warmup)
        if not 0.0 <= warmup < math.inf:
            raise ValueError('WeightEMA: warmup must be a finite number >= 0 (or None), got %r' % (warmup,))
    return decay, warmup


class WeightEMA:
    def __init__(self, module, decay=0.999, warmup=None, follow=None):
        """``warmup``: None = the constant ``decay``; a number w > 0 = ``min(decay, (1 + n) / (w + n))`` for update n = 0, 1, ...
        (short averaging windows first, so the random initial weights wash out quickly).
        ``follow``: a capturable ``optim.Adam``; an update behind a step that optimizer skipped (``skip_nonfinite``) changes
        neither shadows nor count.  It reads the flag of the optimizer's LAST step: call ``update()`` after ``step()``."""
        self.decay, self.warmup = _check_schedule(decay, warmup)
        if follow is not None:
            from .optim import Adam
            if not isinstance(follow, Adam) or not follow._capturable:
                raise ValueError('WeightEMA: follow= takes an optim.Adam(capturable=True): only its skip decision lives on the device')
        self.module, self._follow = module, follow
        params = list(module.named_parameters())
        buffers = list(module.named_buffers())
        if not params:
            raise ValueError('WeightEMA: the module has no parameters')
        for name, p in params:
            E.require_gpu_tensor(p, 'WeightEMA parameter %s' % name)
            if not p.is_contiguous():
                raise RuntimeError('WeightEMA parameter %s: dense contiguous fp32 parameters expected; there is no fallback' % name)
        dev = params[0][1].device
        for name, t in params + buffers:
            if t.device != dev or (t.dtype == torch.float32 and not t.is_contiguous()):
                raise RuntimeError('WeightEMA tensor %s: contiguous tensors on ONE MI355X device expected (got %s); there is no '
                                   'fallback' % (name, t.device))
        self._skip = None
        if follow is not None:
            self._skip = follow.skip_flag
            if self._skip.device != dev:
                raise ValueError('WeightEMA: the followed optimizer lives on %s, the module on %s' % (self._skip.device, dev))
        with torch.no_grad():
            # (name, live, shadow, mode): the launch's tensors -- mode 0 averaged, mode 1 copied; then torch's share
            self._fused = [(k, p, p.detach().clone(), 0) for k, p in params]
            self._fused += [(k, b, b.detach().clone(), 1) for k, b in buffers if b.dtype == torch.float32]
            self._other = [(k, b, b.detach().clone()) for k, b in buffers if b.dtype != torch.float32]
        self._count = torch.zeros((), dtype=torch.int32, device=dev)
        self._ctrl = torch.zeros(2, dtype=torch.float32, device=dev)
        self._table, self._key, self._n, self._blocks = None, None, 0, 0
        self._build_table()

    # ---- descriptor table -------------------------------------------------------------------------------------------
    def _live_key(self):
        return tuple(live.data_ptr() for _, live, _, _ in self._fused)

    def _build_table(self):
        """(re)writes the table IN PLACE: a captured launch holds its address"""
        rows = [r for r in self._fused if r[1].numel() > 0]
        table = (L.EmaDesc * len(rows))()
        for d, (_, live, shadow, mode) in zip(table, rows):
            d.ema, d.src, d.numel, d.mode = shadow.data_ptr(), live.data_ptr(), live.numel(), mode
        blocks = E._fill_block_starts(table)
        staged = E._table_to_device(table, self._count.device)
        if self._table is None:
            self._table = staged
        else:
            self._table.copy_(staged)
        self._key, self._n, self._blocks = self._live_key(), len(rows), blocks

    def _check_addresses(self):
        """the table holds raw pointers: a live tensor that was replaced (``p.data = ...``, ``module.to(...)``) is picked up by
        an eager call; a captured launch cannot follow it"""
        if self._live_key() == self._key:
            return
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('WeightEMA: a live tensor moved since the descriptor table was built; a captured update cannot '
                               'follow it -- call update() once outside the capture first')
        for name, live, shadow, _ in self._fused:
            E.require_gpu_tensor(live, 'WeightEMA tensor %s' % name)
            if not live.is_contiguous() or live.shape != shadow.shape or live.device != shadow.device:
                raise RuntimeError('WeightEMA tensor %s: changed layout, shape or device; there is no fallback' % name)
        self._build_table()

    # ---- the schedule ---------------------------------------------------------------------------------------------------
    def decay_at(self, n):
        """the decay of update number n (0-based), in double: the host restatement of what sisr_ema_prepare computes"""
        if self.warmup is not None and self.warmup > 0.0:
            return min(self.decay, (1.0 + float(n)) / (self.warmup + float(n)))
        return self.decay

    @property
    def num_updates(self):
        """0-dim int32 device tensor: updates applied so far (reading it is the caller's synchronisation)"""
        return self._count

    # ---- update / swap ----------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def update(self):
        lib = L.lib()
        self._check_addresses()
        stream = E._stream()
        L.check(lib.sisr_ema_prepare(self._count.data_ptr(), self.decay, self.warmup or 0.0, E._ptr(self._skip),
                                     self._ctrl.data_ptr(), stream), 'sisr_ema_prepare')
        L.check(lib.sisr_ema_update(self._table.data_ptr(), self._n, self._blocks, self._ctrl.data_ptr(), stream), 'sisr_ema_update')
        if self._other:
            torch._foreach_copy_([s for _, _, s in self._other], [b for _, b, _ in self._other])

    @torch.no_grad()
    def swap(self):
        """live <-> averaged, in place.  Not capturable on purpose: a replayed swap would change parameters with no host call."""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('WeightEMA.swap() inside a stream capture: every replay would exchange the weights again with no '
                               'host call -- swap outside the graph (captured graphs stay valid: no address moves)')
        self._check_addresses()
        L.check(L.lib().sisr_ema_swap(self._table.data_ptr(), self._n, self._blocks, E._stream()), 'sisr_ema_swap')
        if self._other:
            lives, shadows = [b for _, b, _ in self._other], [s for _, _, s in self._other]
            kept = [b.clone() for b in lives]
            torch._foreach_copy_(lives, shadows)
            torch._foreach_copy_(shadows, kept)
        E.invalidate_weight_caches()          # the kernel rewrote parameters behind torch's version counters

    @contextlib.contextmanager
    def applied(self):
        """``with ema.applied(): ...`` -- the module holds the averaged weights inside the block, the live ones again after it
        (also when the block raises)"""
        self.swap()
        try:
            yield self
        finally:
            self.swap()

    # ---- state ------------------------------------------------------------------------------------------------------------
    def _shadow_of(self):
        m = {id(live): shadow for _, live, shadow, _ in self._fused}
        m.update((id(live), shadow) for _, live, shadow in self._other)
        return m

    def shadow_state_dict(self):
        """detached clones of the averaged tensors under exactly the keys of ``module.state_dict()``: loads into a fresh
        module (``load_state_dict``), travels in a checkpoint as ``'net_g_ema'``"""
        shadow_of = self._shadow_of()
        out = OrderedDict()
        for k, live in self.module.state_dict(keep_vars=True).items():
            if id(live) not in shadow_of:
                raise RuntimeError('WeightEMA: %s joined the module after the average was created' % k)
            out[k] = shadow_of[id(live)].detach().clone()
        return out

    def state_dict(self):
        """the shadows themselves (detached, not cloned: as ``nn.Module.state_dict()``), a snapshot of the count, the schedule"""
        shadows = OrderedDict((k, s.detach()) for k, _, s, _ in self._fused)
        shadows.update((k, s) for k, _, s in self._other)
        return dict(shadow=shadows, num_updates=self._count.clone(), decay=self.decay, warmup=self.warmup)

    @torch.no_grad()
    def load_state_dict(self, state):
        """copies INTO the existing tensors (a captured update points at them)"""
        mine = OrderedDict((k, s) for k, _, s, _ in self._fused)
        mine.update((k, s) for k, _, s in self._other)
        theirs = state['shadow']
        if set(mine) != set(theirs):
            raise KeyError('WeightEMA.load_state_dict: tensor names differ: %s' % sorted(set(mine) ^ set(theirs)))
        for k, s in mine.items():
            if s.shape != theirs[k].shape:
                raise ValueError('WeightEMA.load_state_dict: %s has shape %s, the module %s'
                                 % (k, tuple(theirs[k].shape), tuple(s.shape)))
        decay, warmup = _check_schedule(state['decay'], state['warmup'])
        for k, s in mine.items():
            s.copy_(theirs[k])
        self._count.copy_(torch.as_tensor(state['num_updates'], dtype=torch.int32).reshape(()))
        self.decay, self.warmup = decay, warmup
