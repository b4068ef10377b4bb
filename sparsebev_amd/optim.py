"""FusedAdamW: the training recipe's parameter update -- AdamW, gradient clipping by global L2 norm, a static loss scale, the step
skipped when the gradients are not finite -- as THREE launches of csrc/optim.hip over all parameters, without a host synchronisation,
so that it can be the tail of a captured train step (train_graph.CapturedTrainStep / CapturedHeadTrainStep ``optimizer=``).

Reference counterpart: ``optimizer = dict(type='AdamW', lr=2e-4, paramwise_cfg=dict(custom_keys={'sampling_offset': dict(lr_mult=0.1)}),
weight_decay=0.01)`` and ``optimizer_config = dict(type='Fp16OptimizerHook', loss_scale=512.0, grad_clip=dict(max_norm=35, norm_type=2))``
(configs/r50_nuimg_704x256.py:186-200): with torch that is clip_grad_norm_ + AdamW.step, dozens of small launches over the head's 51
parameter tensors, and either not capturable or synchronising.

What a step reads:
  * addresses and sizes of p / grad / exp_avg / exp_avg_sq: host tables that travel by value in the launches (rebuilt when a ``.grad``
    address changes -- eager backward hands over new buffers every step; a capture bakes them into its nodes);
  * lr, weight_decay and lr multiplier per group, 1 / loss_scale, max_grad_norm, the hold word: one small device buffer at a fixed
    address, refreshed from ``param_groups`` by one pinned asynchronous copy when something changed (LR schedulers that write
    ``group['lr']`` work unchanged) -- outside any capture;
  * the step counter and the running beta powers: a device header that only the middle launch writes.
``grad_norm``, ``skipped`` and ``step_count`` are device tensors (views of the header): reading them is the caller's synchronisation.
"""
import ctypes

import torch

from . import _lib

CHUNK = 8192            # SBEV_OPTIM_CHUNK
MAX_TENSORS = 64        # SBEV_OPTIM_MAX_TENSORS: per launch
MAX_GROUPS = 16         # SBEV_OPTIM_MAX_GROUPS
_HYPER_FLOATS = 68      # SBEV_OPTIM_HYPER_FLOATS
_HEADER_BYTES = 64      # SBEV_OPTIM_HEADER_BYTES


def plan(numels):
    """(chunks, launches, workspace bytes) of a list of element counts: sbev_optim_plan, a pure host function."""
    n = len(numels)
    arr = (ctypes.c_int64 * max(n, 1))(*[int(v) for v in numels])
    out = (ctypes.c_int64 * 3)()
    _lib.check(_lib.load().sbev_optim_plan(arr, n, out), 'sbev_optim_plan')
    return int(out[0]), int(out[1]), int(out[2])


def param_groups(named_parameters, lr, weight_decay, custom_keys=None):
    """Parameter groups by the rule of mmcv's DefaultOptimizerConstructor (paramwise_cfg.custom_keys): the keys are sorted
    alphabetically and then by length, longest first; the FIRST key that is a substring of a parameter's name decides, and sets
    ``lr = lr * lr_mult`` and ``weight_decay = weight_decay * decay_mult`` (each default 1).  Parameters that do not require grad are
    left out.  Parameters with equal (lr, weight_decay) share a group, in order of first appearance; each group carries ``names``.
    ``param_groups(head.named_parameters(), 2e-4, 0.01, {'sampling_offset': dict(lr_mult=0.1)})`` is the reference's recipe."""
    custom_keys = dict(custom_keys or {})
    keys = sorted(sorted(custom_keys), key=len, reverse=True)
    groups = {}
    for name, p in named_parameters:
        if not p.requires_grad:
            continue
        g_lr, g_wd = lr, weight_decay
        for key in keys:
            if key in name:
                g_lr = lr * custom_keys[key].get('lr_mult', 1.0)
                g_wd = weight_decay * custom_keys[key].get('decay_mult', 1.0)
                break
        g = groups.setdefault((g_lr, g_wd), {'params': [], 'names': [], 'lr': g_lr, 'weight_decay': g_wd})
        g['params'].append(p)
        g['names'].append(name)
    return list(groups.values())


class FusedAdamW(torch.optim.Optimizer):
    """``FusedAdamW(params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=None, loss_scale=1.0)``.

    ``step()`` = unscale by ``loss_scale``, clip to ``max_grad_norm`` (None: off), AdamW as torch defines it, all skipped when the
    gradient norm is not finite (``skipped`` counts those; the step counter and the moments do not move).  A group may carry
    ``lr_mult`` (default 1): the device multiplies it into ``lr``.  ``betas`` and ``eps`` are one setting for all groups (the beta
    powers have one counter).  ``max_grad_norm`` and ``loss_scale`` are attributes and may be changed between steps.
    ``state_dict()`` / ``load_state_dict()`` speak torch.optim.AdamW's format, so a checkpoint moves between the two."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, maximize=False,
                 max_grad_norm=None, loss_scale=1.0):
        if amsgrad:
            raise ValueError('FusedAdamW: amsgrad is not implemented')
        if maximize:
            raise ValueError('FusedAdamW: maximize is not implemented')
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0) or eps < 0.0 or lr < 0.0 or weight_decay < 0.0:
            raise ValueError('FusedAdamW: need 0 <= beta < 1, eps >= 0, lr >= 0, weight_decay >= 0')
        self._ready = False
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, lr_mult=1.0)
        super().__init__(params, defaults)
        self.max_grad_norm = max_grad_norm
        self.loss_scale = float(loss_scale)
        self.hold = False               # True: every step is skipped (the captured steps' warm-up)
        self.device = self.param_groups[0]['params'][0].device
        if len(self.param_groups) > MAX_GROUPS:
            raise ValueError('FusedAdamW: %d parameter groups (at most %d)' % (len(self.param_groups), MAX_GROUPS))
        header = torch.zeros(_HEADER_BYTES, dtype=torch.uint8, device=self.device)
        self._header = header
        self._beta_pows = header[0:16].view(torch.float64)
        self._beta_pows.fill_(1.0)
        self.step_count = header[16:24].view(torch.int64)[0]         # device views: reading them synchronises the reader
        self.skipped = header[24:32].view(torch.int64)[0]
        self.grad_norm = header[32:36].view(torch.float32)[0]
        self.clip_coef = header[36:40].view(torch.float32)[0]
        self._hyper = torch.zeros(_HYPER_FLOATS, dtype=torch.float32, device=self.device)
        self._hyper_host = torch.zeros(_HYPER_FLOATS, dtype=torch.float32).pin_memory()
        self._hyper_sent = None
        self._hyper_event = None
        self._tables = None
        self._table_key = None
        self._partials = None
        for group in self.param_groups:
            for p in group['params']:
                self.state[p] = {'exp_avg': torch.zeros_like(p), 'exp_avg_sq': torch.zeros_like(p)}
        self._ready = True

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        group = self.param_groups[-1]
        for p in group['params']:
            if not p.is_cuda:
                raise RuntimeError('FusedAdamW needs device parameters (no CPU fallback)')
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise ValueError('FusedAdamW: parameters must be contiguous fp32 tensors (got %s, contiguous=%s)' % (p.dtype, p.is_contiguous()))
        if group.get('amsgrad') or group.get('maximize'):
            raise ValueError('FusedAdamW: amsgrad / maximize are not implemented')
        if self._ready:                 # a group added after construction
            if len(self.param_groups) > MAX_GROUPS:
                raise ValueError('FusedAdamW: %d parameter groups (at most %d)' % (len(self.param_groups), MAX_GROUPS))
            for p in group['params']:
                if p.device != self.device:
                    raise ValueError('FusedAdamW: all parameters must live on one device')
                self.state[p] = {'exp_avg': torch.zeros_like(p), 'exp_avg_sq': torch.zeros_like(p)}
            self._table_key = None

    # ---- the device buffer of what changes between steps
    def _hyper_values(self):
        b0 = self.param_groups[0]
        vals = [1.0 / self.loss_scale, -1.0 if self.max_grad_norm is None else float(self.max_grad_norm), 1.0 if self.hold else 0.0, 0.0]
        for g in self.param_groups:
            if tuple(g['betas']) != tuple(b0['betas']) or g['eps'] != b0['eps']:
                raise ValueError('FusedAdamW: betas and eps are one setting for all groups')
            vals += [float(g['lr']), float(g['weight_decay']), float(g.get('lr_mult', 1.0)), 0.0]
        return tuple(vals)

    def push_hyper(self):
        """Bring the device buffer up to date with ``param_groups``, ``loss_scale``, ``max_grad_norm`` and ``hold``: one pinned
        asynchronous copy on the current stream when something changed, nothing otherwise.  Never under a capture: a captured step's
        ``replay`` calls this in front of the graph."""
        vals = self._hyper_values()
        if vals == self._hyper_sent:
            return
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('FusedAdamW: lr / weight_decay / loss_scale / max_grad_norm changed while the stream is capturing; the upload '
                               'belongs in front of the capture (push_hyper())')
        if self._hyper_event is not None:
            self._hyper_event.synchronize()          # the last upload has left the pinned buffer (it was enqueued a step ago)
        self._hyper_host[:len(vals)] = torch.tensor(vals, dtype=torch.float32)
        self._hyper.copy_(self._hyper_host, non_blocking=True)
        self._hyper_event = torch.cuda.Event()
        self._hyper_event.record()
        self._hyper_sent = vals

    # ---- the by-value tables
    def _params(self):
        return [(p, gi) for gi, g in enumerate(self.param_groups) for p in g['params']]

    def _build_tables(self):
        plist = self._params()
        for p, _ in plist:
            if p.grad is None:
                raise RuntimeError('FusedAdamW.step: a parameter has no .grad (run backward first; freeze a parameter with requires_grad=False '
                                   'before building the optimizer)')
            if p.grad.dtype != torch.float32 or not p.grad.is_contiguous() or p.grad.device != p.device:
                raise ValueError('FusedAdamW.step: gradients must be contiguous fp32 tensors on the parameters\' device')
        key = tuple((p.data_ptr(), p.grad.data_ptr(), self.state[p]['exp_avg'].data_ptr(), self.state[p]['exp_avg_sq'].data_ptr()) for p, _ in plist)
        if key == self._table_key:
            return
        VP = ctypes.c_void_p
        tables, base = [], 0
        for first in range(0, len(plist), MAX_TENSORS):
            part = plist[first:first + MAX_TENSORS]
            n = len(part)
            numels = [p.numel() for p, _ in part]
            chunks = plan(numels)[0]
            tables.append(dict(
                n=n, base=base, chunks=chunks,
                p=(VP * n)(*[p.data_ptr() for p, _ in part]), g=(VP * n)(*[p.grad.data_ptr() for p, _ in part]),
                m=(VP * n)(*[self.state[p]['exp_avg'].data_ptr() for p, _ in part]),
                v=(VP * n)(*[self.state[p]['exp_avg_sq'].data_ptr() for p, _ in part]),
                numel=(ctypes.c_int64 * n)(*numels), group=(ctypes.c_int32 * n)(*[gi for _, gi in part])))
            base += chunks
        self._tables, self._chunks, self._table_key = tables, base, key
        if self._partials is None or self._partials.numel() < max(base, 1):
            self._partials = torch.empty(max(base, 1), dtype=torch.float32, device=self.device)

    def enqueue(self):
        """The three launches on the current stream (tables rebuilt on the host when an address changed).  No upload, no version bump."""
        self._build_tables()
        lib = _lib.load()
        stream = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        hyper, header = ctypes.c_void_p(self._hyper.data_ptr()), ctypes.c_void_p(self._header.data_ptr())
        b1, b2 = self.param_groups[0]['betas']
        eps = self.param_groups[0]['eps']
        for t in self._tables:
            part = ctypes.c_void_p(self._partials.data_ptr() + 4 * t['base'])
            _lib.check(lib.sbev_optim_sumsq(t['g'], t['numel'], t['n'], hyper, part, stream), 'sbev_optim_sumsq')
        _lib.check(lib.sbev_optim_finish(ctypes.c_void_p(self._partials.data_ptr()), self._chunks, hyper, header, b1, b2, stream), 'sbev_optim_finish')
        for t in self._tables:
            _lib.check(lib.sbev_optim_adamw(t['p'], t['g'], t['m'], t['v'], t['numel'], t['group'], t['n'], len(self.param_groups),
                                            b1, b2, eps, hyper, header, stream), 'sbev_optim_adamw')

    def bump_versions(self):
        """The launches write through raw pointers: tell everything that watches ``_version`` (the cached weight images of
        sparsebev_amd.autograd / dense, the inference runtime's packed images and step-graph signature) that the parameters moved."""
        torch.autograd.graph.increment_version([p for p, _ in self._params()])

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if not torch.cuda.is_current_stream_capturing():
            self.push_hyper()
        elif self._hyper_sent is None:
            raise RuntimeError('FusedAdamW.step under a capture before the first push_hyper()')
        self.enqueue()
        self.bump_versions()
        return loss

    # ---- torch.optim.AdamW's state format
    def state_dict(self):
        """torch.optim.AdamW's: per parameter ``step`` (the one counter, read from the device: this synchronises), ``exp_avg``,
        ``exp_avg_sq``; plus the groups."""
        step = float(self.step_count.item())
        sd = super().state_dict()
        sd['state'] = {k: dict(step=torch.tensor(step, dtype=torch.float32), **s) for k, s in sd['state'].items()}
        return sd

    def load_state_dict(self, state_dict):
        """From a FusedAdamW or a torch.optim.AdamW state.  The moments are copied INTO this optimizer's own tensors (a captured step
        holds their addresses).  ``ValueError`` when the parameters' ``step`` values differ: there is one counter."""
        steps = {float(s['step']) for s in state_dict['state'].values() if 'step' in s}
        if len(steps) > 1:
            raise ValueError('FusedAdamW.load_state_dict: the parameters\' step values differ (%s); this optimizer keeps one counter' % sorted(steps))
        own = {p: (self.state[p]['exp_avg'], self.state[p]['exp_avg_sq']) for p, _ in self._params()}
        super().load_state_dict(state_dict)
        t = int(steps.pop()) if steps else 0
        for g in self.param_groups:
            g.setdefault('lr_mult', 1.0)
        for p, (m, v) in own.items():
            new = self.state.get(p, {})
            m.copy_(new['exp_avg']) if 'exp_avg' in new else m.zero_()
            v.copy_(new['exp_avg_sq']) if 'exp_avg_sq' in new else v.zero_()
            self.state[p] = {'exp_avg': m, 'exp_avg_sq': v}
        b1, b2 = self.param_groups[0]['betas']
        p1 = p2 = 1.0
        for _ in range(t):              # the device's running products: one fp64 multiplication per step
            p1, p2 = p1 * b1, p2 * b2
        self._beta_pows.copy_(torch.tensor([p1, p2], dtype=torch.float64))
        self._header[16:24].view(torch.int64).fill_(t)
        self._hyper_sent = None
