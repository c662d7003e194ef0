"""Fused Adam for the MI355X path.

Drop-in for the optimizer the reference builds, ``optim.Adam(net.parameters(), lr=lr, betas=(.9, 0.999))``
(config.py:292-294), stepped once per network per iteration (train.py:75,108) and driven by ``LambdaLR``
(config.py:170-180; train.py:121-122).  Subclasses ``torch.optim.Adam`` so the constructor, ``param_groups``,
``state_dict()`` / ``load_state_dict()`` (the reference checkpoints ``opti_g`` / ``opti_d``, utils.py:108-115) and
schedulers behave as before; only ``step()`` differs: ONE HIP launch (``sisr_adam_step``) updates every parameter
of a group instead of several elementwise passes per tensor list.  Device fp32 parameters only, no fallback.

``capturable=True`` keeps every per-step scalar on the device, so that ``step()`` can sit inside a
captured HIP graph (graph.GraphedStep) and still advance on every replay:

* ``state[p]['step']`` is a 0-dim fp32 DEVICE tensor (torch's capturable layout), a view into one block per optimizer;
  a small prepare launch turns it into the step's bias corrections and adds one.  ``step()`` never reads it back.
* ``group['lr']`` may be a Python float or a 1-element device tensor (fp32 or fp64).  A tensor is read in place by the
  kernels: torch's schedulers ``fill_`` a tensor ``lr``, so ``LambdaLR`` works across replays with nothing else to call --
  UNDER REPLAY USE THE TENSOR FORM.  A float is mirrored into a device scalar that an EAGER ``step()`` refreshes
  (without a host synchronisation) whenever the float changed; a replayed step keeps reading the value of the last
  eager step.
* ``max_grad_norm`` (global-norm clipping with ``clip_grad_norm_``'s formula; the gradients themselves are not modified)
  and ``skip_nonfinite`` (a step whose gradient norm is not finite changes nothing and is counted) add one read of the
  gradients; both imply ``capturable``.  ``grad_norm`` and ``skipped_steps`` are 0-dim device tensors: reading them is the
  caller's synchronisation, not the optimizer's.
* Addresses never change after the first ``step()`` (a captured step holds raw pointers): moments, step counts, control
  block and constants are allocated then -- in a warm-up run, never inside a capture; ``load_state_dict`` copies INTO the
  existing tensors and ``zero_state()`` resets them in place (``state.clear()`` would orphan a captured step)."""
import ctypes as C
import math

import torch

from . import _lib as L
from . import engine as E


class Adam(torch.optim.Adam):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, capturable=False,
                 max_grad_norm=None, skip_nonfinite=False, **kw):
        if amsgrad or kw.get('maximize') or kw.get('differentiable'):
            raise NotImplementedError('fused Adam: amsgrad / maximize / differentiable are not implemented '
                                      '(the reference uses none of them, config.py:292-294)')
        if max_grad_norm is not None and not float(max_grad_norm) >= 0.0:
            raise ValueError('fused Adam: max_grad_norm must be >= 0, got %r' % (max_grad_norm,))
        kw.pop('foreach', None)
        kw.pop('fused', None)
        self._capturable = bool(capturable or max_grad_norm is not None or skip_nonfinite)
        self._max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self._skip_nonfinite = bool(skip_nonfinite)
        if self._capturable:
            kw['capturable'] = True
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, **kw)
        self._tables = {}
        self._dev = None                   # device-state buffers, allocated by the first capturable step()
        self._moments = {}                 # parameter -> (exp_avg, exp_avg_sq): outlives state entries, addresses are final
        self._captured = []                # tables staged inside a capture: the graph re-reads them on every replay

    # ---- state dicts ----------------------------------------------------------------------------------------
    def load_state_dict(self, state_dict):
        if not self._capturable:
            super().load_state_dict(state_dict)
            self._tables = {}                  # the cached descriptor tables point at the replaced moment tensors
            for st in self.state.values():     # 'step' stays a host scalar (torch moves it to the parameter's device)
                if isinstance(st.get('step'), torch.Tensor) and st['step'].is_cuda:
                    st['step'] = st['step'].cpu()
            return
        # capturable: whatever the state dict comes from (torch's Adam, capturable or not, or the host-state fused Adam, 'step'
        # a host or a device tensor), its values are copied INTO the tensors a captured step points at
        lrs = [g['lr'] for g in self.param_groups]
        super().load_state_dict(state_dict)
        for g, lr in zip(self.param_groups, lrs):
            g['capturable'] = True
            if isinstance(lr, torch.Tensor):   # the kernels read THIS tensor: keep it, with the loaded value
                lr.fill_(float(g['lr']))
                g['lr'] = lr
        loaded = {p: st for p, st in self.state.items() if len(st)}
        if not loaded:
            return
        self._allocate(next(iter(loaded)).device)
        for p, st in loaded.items():
            m, v = self._moments_of(p)
            if m.shape == st['exp_avg'].shape and v.shape == st['exp_avg_sq'].shape:
                m.copy_(st['exp_avg'])
                v.copy_(st['exp_avg_sq'])
            else:
                raise ValueError('fused Adam: loaded moments of shape %s for a parameter of shape %s'
                                 % (tuple(st['exp_avg'].shape), tuple(p.shape)))
            step = self._dev['steps'][self._dev['index'][p]]
            step.copy_(torch.as_tensor(st['step'], dtype=torch.float32).reshape(()))
            st['step'], st['exp_avg'], st['exp_avg_sq'] = step, m, v

    def state_dict(self):
        sd = super().state_dict()
        if self._capturable and self._dev is not None:
            # the step counts are views into ONE live block that the kernels advance: hand out a snapshot (state ids follow the
            # order of param_groups, which is the order of the block)
            steps = self._dev['steps'].clone()
            sd['state'] = {k: dict(st, step=steps[k]) if 'step' in st else st for k, st in sd['state'].items()}
        return sd

    def __setstate__(self, state):
        super().__setstate__(state)
        self._tables = {}
        if '_capturable' not in self.__dict__:          # unpickled: Optimizer.__getstate__ keeps defaults, state and param_groups only
            self._capturable = any(g.get('capturable') for g in self.param_groups)
            self._max_grad_norm, self._skip_nonfinite = None, False
            self._dev, self._moments, self._captured = None, {}, []

    def zero_state(self):
        """Capturable mode: zero moments, step counts and the control block IN PLACE (the restart from scratch that
        ``state.clear()`` is for the host-state optimizer, without moving anything a captured step points at)."""
        if not self._capturable:
            raise RuntimeError('fused Adam: zero_state() belongs to capturable=True (use state.clear() otherwise)')
        for m, v in self._moments.values():
            m.zero_()
            v.zero_()
        if self._dev is not None:
            self._dev['steps'].zero_()
            self._dev['ctrl'].zero_()

    # ---- device state -----------------------------------------------------------------------------------------
    def _allocate(self, device):
        if self._dev is not None:
            return
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('fused Adam(capturable=True): the first step() allocates the optimizer state and cannot run inside '
                               'a stream capture -- run a warm-up step first (graph.GraphedStep does)')
        lib = L.lib()
        params = [p for g in self.param_groups for p in g['params']]
        blocks = E._fill_block_starts((L.AdamDesc * len(params))(*[L.AdamDesc(numel=p.numel()) for p in params]))
        ctrl = torch.zeros(4, dtype=torch.float32, device=device)
        self._dev = {
            'index': {p: i for i, p in enumerate(params)},
            'steps': torch.zeros(len(params), dtype=torch.float32, device=device),
            'ctrl': ctrl, 'norm': ctrl[0], 'skip': ctrl.view(torch.int32)[2], 'skipped': ctrl.view(torch.int32)[3],
            'consts': [torch.zeros(2 * len(g['params']), dtype=torch.float32, device=device) for g in self.param_groups],
            'partials': torch.zeros(max(1, L.check_count(lib.sisr_adam_norm_ws_doubles(max(1, blocks)), 'sisr_adam_norm_ws_doubles')),
                                    dtype=torch.float64, device=device),
            'lr': [None] * len(self.param_groups), 'lr_value': [None] * len(self.param_groups),
        }

    def _moments_of(self, p):
        mv = self._moments.get(p)
        if mv is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError('fused Adam(capturable=True): a parameter receives its first gradient inside a stream capture; '
                                   'its moments must be allocated by a warm-up step outside the capture')
            mv = self._moments[p] = (torch.zeros_like(p, memory_format=torch.preserve_format),
                                     torch.zeros_like(p, memory_format=torch.preserve_format))
        return mv

    def _lr_scalar(self, gi, group, device):
        """(device tensor, is_fp64) the kernels read the group's learning rate from"""
        lr = group['lr']
        if isinstance(lr, torch.Tensor):
            if not lr.is_cuda or lr.numel() != 1 or lr.dtype not in (torch.float32, torch.float64):
                raise RuntimeError('fused Adam(capturable=True): a tensor lr must be ONE fp32 or fp64 element on the device')
            return lr, lr.dtype == torch.float64
        d = self._dev
        value = float(lr)
        if d['lr_value'][gi] != value and not torch.cuda.is_current_stream_capturing():
            if d['lr'][gi] is None:
                d['lr'][gi] = torch.zeros(1, dtype=torch.float64, device=device)
            staged = E._table_to_device((C.c_double * 1)(value), device)           # pinned staging: no host synchronisation
            d['lr'][gi].copy_(staged[:8].view(torch.float64))
            d['lr_value'][gi] = value
        if d['lr'][gi] is None:
            raise RuntimeError('fused Adam(capturable=True): no device copy of the float lr yet -- run a warm-up step outside the capture')
        return d['lr'][gi], True

    @property
    def grad_norm(self):
        """0-dim device tensor: the global gradient norm of the last step that ran a guard (0 before)"""
        return self._readout('norm')

    @property
    def skipped_steps(self):
        """0-dim int32 device tensor: steps skipped so far because their gradient norm was not finite"""
        return self._readout('skipped')

    @property
    def skip_flag(self):
        """0-dim int32 device tensor: 1 while the LAST step was skipped (non-finite norm under ``skip_nonfinite``), else 0 -- the
        word the step kernel itself tests; a kernel that must follow the optimizer's decision (ema.WeightEMA(follow=...)) reads it"""
        return self._readout('skip')

    def _readout(self, key):
        if not self._capturable:
            raise RuntimeError('fused Adam: grad_norm / skipped_steps / skip_flag belong to capturable=True')
        if self._dev is None:
            self._allocate(self.param_groups[0]['params'][0].device)
        return self._dev[key]

    # ---- steps ----------------------------------------------------------------------------------------------------
    @staticmethod
    def _refuse(p):
        E.require_gpu_tensor(p, 'fused Adam parameter')
        if p.grad.is_sparse or p.grad.dtype != torch.float32 or not p.is_contiguous():
            raise RuntimeError('fused Adam: dense contiguous fp32 parameters and gradients expected')

    def _table(self, gi, plist):
        """(device table, total blocks, gradients) of group gi's launch over plist.  The staged buffer holds the descriptor table
        and, in capturable mode, the step-count pointers behind it (48 n bytes in: 8-byte aligned).  It holds raw pointers of
        parameters, gradients, both moment tensors and step counts: all of them are the cache key (load_state_dict() replaces
        the moments of the host-state optimizer at unchanged parameter / gradient addresses).  The returned gradients keep
        contiguous copies alive until the launch is issued."""
        grads = [p.grad if p.grad.is_contiguous() else p.grad.contiguous() for p in plist]
        states = [self.state[p] for p in plist]
        rows = [(p.data_ptr(), st['exp_avg'].data_ptr(), st['exp_avg_sq'].data_ptr(), g.data_ptr(), p.numel())          # AdamDesc
                for p, st, g in zip(plist, states, grads)]
        steps = [st['step'].data_ptr() for st in states] if self._capturable else []
        key = (rows, steps)
        capturing = self._capturable and torch.cuda.is_current_stream_capturing()
        cached = None if capturing else self._tables.get(gi)
        if cached is None or cached[0] != key:
            table = (L.AdamDesc * len(rows))(*[L.AdamDesc(*r) for r in rows])
            blocks = E._fill_block_starts(table)
            staged = E._table_to_device(bytes(table) + bytes((C.c_void_p * len(steps))(*steps)), plist[0].device)
            cached = (key, staged, blocks)
            if capturing:
                self._captured.append(cached)          # the graph re-reads the staged table on every replay
            else:
                self._tables[gi] = cached
        return cached[1], cached[2], grads

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self._capturable:
            self._step_capturable()
            return loss
        lib = L.lib()
        E.invalidate_weight_caches()      # the kernel below rewrites parameters behind torch's version counters
        for gi, group in enumerate(self.param_groups):
            by_step = {}
            for p in group['params']:
                if p.grad is None:
                    continue
                self._refuse(p)
                st = self.state[p]
                if len(st) == 0:          # same state layout as torch.optim.Adam
                    st['step'] = torch.tensor(0.0, dtype=torch.float32)
                    st['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st['step'] += 1
                by_step.setdefault(int(st['step'].item()), []).append(p)     # 'step' lives on the host: no sync
            beta1, beta2 = group['betas']
            for t, plist in by_step.items():
                table, blocks, grads = self._table(gi, plist)
                L.check(lib.sisr_adam_step(table.data_ptr(), len(plist), blocks, float(group['lr']), beta1, beta2,
                                           group['eps'], group['weight_decay'], 1.0 - math.pow(beta1, t),
                                           1.0 - math.pow(beta2, t), E._stream()), 'sisr_adam_step')
                del grads
        return loss

    def _step_capturable(self):
        """[sum of squares per group] -> prepare per group -> step per group; a group whose parameters have no gradient is left
        out, and so is a parameter without one (its count lags, as in the host-state step)"""
        from . import graph as G
        lib = L.lib()
        guard = self._max_grad_norm is not None or self._skip_nonfinite
        for group in self.param_groups:      # refusals first: nothing below may look for a device on behalf of a CPU tensor
            for p in group['params']:
                if p.grad is not None:
                    self._refuse(p)
        capturing = torch.cuda.is_current_stream_capturing()
        work = []
        for gi, group in enumerate(self.param_groups):
            plist = [p for p in group['params'] if p.grad is not None]
            if not plist:
                continue
            self._allocate(plist[0].device)
            d = self._dev
            for p in plist:
                st = self.state[p]
                if len(st) == 0:          # torch.optim.Adam(capturable=True)'s state layout
                    m, v = self._moments_of(p)
                    st['step'], st['exp_avg'], st['exp_avg_sq'] = d['steps'][d['index'][p]], m, v
            work.append((gi, group, plist) + self._table(gi, plist))
        if not work:
            return
        E.invalidate_weight_caches()      # the step kernel rewrites parameters behind torch's version counters
        if capturing and G._ACTIVE is not None:
            G._ACTIVE.captures_optimizer = True          # its replays change parameters with no host call: see graph.py
        d, stream = self._dev, E._stream()
        n_part = 0
        if guard:
            for gi, group, plist, table, blocks, grads in work:
                L.check(lib.sisr_adam_grad_sumsq(table.data_ptr(), len(plist), blocks,
                                                 d['partials'].data_ptr() + 8 * n_part, stream), 'sisr_adam_grad_sumsq')
                n_part += blocks
        max_norm = -1.0 if self._max_grad_norm is None else self._max_grad_norm
        for k, (gi, group, plist, table, blocks, grads) in enumerate(work):
            lr, lr_f64 = self._lr_scalar(gi, group, plist[0].device)
            beta1, beta2 = group['betas']
            L.check(lib.sisr_adam_prepare(table.data_ptr() + C.sizeof(L.AdamDesc) * len(plist), len(plist), lr.data_ptr(),
                                          int(lr_f64), beta1, beta2, d['partials'].data_ptr() if n_part else None, n_part, max_norm,
                                          int(self._skip_nonfinite), int(k == 0), d['ctrl'].data_ptr(), d['consts'][gi].data_ptr(),
                                          stream), 'sisr_adam_prepare')
        for gi, group, plist, table, blocks, grads in work:
            beta1, beta2 = group['betas']
            L.check(lib.sisr_adam_step_dev(table.data_ptr(), len(plist), blocks, d['consts'][gi].data_ptr(), d['ctrl'].data_ptr(),
                                           beta1, beta2, group['eps'], group['weight_decay'], stream), 'sisr_adam_step_dev')
