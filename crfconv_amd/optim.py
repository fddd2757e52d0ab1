"""Flat-buffer SGD for the training step of trainval.py:69-73,105 (torch.optim.SGD with momentum and weight decay,
wrapped by ExponentialLR).

All parameters of the model become views of ONE contiguous float32 vector, their gradients views of the
``FlatGradAllReduce`` bucket, and the update is a single kernel launch (csrc/optim.hip: sgd_hyper_kernel) instead of the
~15 multi-tensor launches of the framework optimizer.  Same arithmetic, same state (one momentum buffer).

It IS a ``torch.optim.Optimizer``: ``param_groups[0]['lr']`` is the learning rate, so
``torch.optim.lr_scheduler.ExponentialLR(opt, gamma)`` (trainval.py:73) wraps it unchanged.  The kernel reads
{lr, momentum, dampening, weight_decay} from a 4-float DEVICE tensor that ``step()`` refreshes whenever the group's
values changed; when ``step()`` has been captured into a hipGraph the host code no longer runs, so call
``push_hyper()`` after ``scheduler.step()`` (outside the graph) and the next replay uses the new rate.

Difference from torch.optim.SGD, by construction of the flat vector: weight decay and momentum are applied to every
element each step, also to a parameter whose ``.grad`` was None that step (torch skips such a parameter).  Every
parameter of the networks in crfconv_amd.models receives a gradient each step, so the two agree there
(tests/test_gpu_model.py::test_flat_sgd_matches_torch_sgd).

``FlatAdam`` / ``FlatAdamW`` (below) are the same construction for trainval.py:66-68 (the Adam line the reference keeps one
comment away): torch.optim.Adam's arithmetic over the flat vector, with the step count in device memory."""
import ctypes

import torch

from . import _lib
from .graph import ptr, require_gpu, stream_ptr


def _rehome(bucket, who):
    """One contiguous float32 vector holding every parameter of `bucket` (values preserved); each ``p.data`` becomes its view."""
    params = bucket.params
    require_gpu(*params)
    if any(p.dtype != torch.float32 for p in params):
        raise _lib.CrfConvError('%s: float32 parameters only' % who)
    flat = torch.empty_like(bucket.flat)
    o = 0
    for p in params:
        view = flat[o:o + p.numel()].view_as(p)
        view.copy_(p.data)
        p.data = view
        o += p.numel()
    return flat


def _guard_words(dev):
    """(host array of the device's sticky grid-barrier failure words, their count) for the guarded update entries."""
    from . import ops
    ops.gridsync_ws(dev)                                     # (creates this stream's words and the capture buffer on first use)
    words = ops.fail_word_ptrs(dev)
    arr = (ctypes.c_void_p * max(len(words), 1))(*words)
    return arr, len(words)


class FlatSGD(torch.optim.Optimizer):
    def __init__(self, bucket, lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, check_every=64, grad_scale=1.0):
        """`bucket`: distributed.FlatGradAllReduce of the model (owns the flat gradient vector).  check_every: eager steps
        between two host reads of the grid-barrier failure flag (ops.check_gridsync; 0 = never -- the update kernel itself
        reads the flag every step and skips the update while it is set, so nothing is lost in between).  grad_scale: factor on the
        gradient inside the update -- 1 / world size after ``bucket.allreduce_sum()`` (no separate averaging pass)."""
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError('Nesterov momentum requires a momentum and zero dampening')
        self.bucket = bucket
        params = bucket.params
        self.flat = _rehome(bucket, 'FlatSGD')   # re-home every parameter inside the flat vector (values preserved)
        self.buf = torch.zeros_like(self.flat)
        self.steps = 0
        self.check_every = int(check_every)
        self.grad_scale = float(grad_scale)
        super().__init__(params, dict(lr=float(lr), momentum=float(momentum), dampening=float(dampening),
                                      weight_decay=float(weight_decay), nesterov=bool(nesterov)))
        self._hyper = torch.zeros(5, dtype=torch.float32, device=self.flat.device)
        self._hyper_host = None
        self.push_hyper()

    # convenience mirrors of the single parameter group
    @property
    def lr(self):
        return self.param_groups[0]['lr']

    @lr.setter
    def lr(self, value):
        self.param_groups[0]['lr'] = float(value)

    def add_param_group(self, group):
        if getattr(self, 'param_groups', None):
            raise _lib.CrfConvError('FlatSGD keeps ONE parameter group (one flat vector, one launch)')
        super().add_param_group(group)

    def push_hyper(self):
        """Copies the group's {lr, momentum, dampening, weight_decay} (and grad_scale) to the device block the kernel reads, if they
        changed.  step() does this itself when run eagerly; call it explicitly between replays of a captured step."""
        g = self.param_groups[0]
        cur = (float(g['lr']), float(g['momentum']), float(g['dampening']), float(g['weight_decay']), float(self.grad_scale))
        if cur != self._hyper_host:
            self._hyper.copy_(torch.tensor(cur, dtype=torch.float32), non_blocking=False)
            self._hyper_host = cur

    def zero_grad(self, set_to_none=True):
        self.bucket.zero()

    @torch.no_grad()
    def step(self, closure=None):
        """Expects the gradients in bucket.flat: ``bucket.allreduce_mean()`` (any world size) or ``bucket.pack()``
        puts them there after backward."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        g = self.param_groups[0]
        capturing = torch.cuda.is_current_stream_capturing()
        first = self.steps == 0 and g['dampening'] != 0
        if capturing and g['dampening'] != 0:
            raise _lib.CrfConvError('FlatSGD: dampening != 0 makes the first step special; capture is not supported')
        if not capturing:
            self.push_hyper()
        # the update is guarded by EVERY sticky grid-barrier failure word of this device (the stream this step runs on, other
        # eager streams, the buffer captured graphs use -- an eager step() behind a captured forward / backward sees that one too)
        # and by the bucket's guard slot, which under data parallelism holds the ranks' REDUCED flag (FlatGradAllReduce.
        # publish_guard): a step in which a one-launch kernel timed out anywhere (NaN-poisoned outputs -> NaN gradient, summed into
        # every rank's bucket) leaves parameters and momentum untouched on ALL ranks, in eager steps and captured replays alike,
        # until check_gridsync reports it
        arr, nwords = _guard_words(self.flat.device)
        guard = getattr(self.bucket, 'guard', None)
        _lib.call('crfconv_sgd_step_guarded_all', ptr(self.flat), ptr(self.bucket.flat), ptr(self.buf), self.flat.numel(),
                  ptr(self._hyper), 1 if g['nesterov'] else 0, 1 if first else 0, arr, nwords,
                  ptr(guard), stream_ptr())   # zero buffer: mu * 0 + g = g
        self.steps += 1
        if not capturing and self.check_every > 0 and self.steps % self.check_every == 0:
            # raises on EVERY rank when any rank failed (the reduced slot); the guarded updates since the failure changed nothing
            from . import ops
            ops.check_gridsync(self.flat.device, reduced_flag=getattr(self.bucket, 'guard', None))
        return loss

    def state_dict(self):
        sd = super().state_dict()
        sd['flat_momentum'] = self.buf.clone()
        sd['flat_steps'] = self.steps
        return sd

    def load_state_dict(self, sd):
        sd = dict(sd)
        buf = sd.pop('flat_momentum', None)
        self.steps = int(sd.pop('flat_steps', self.steps))
        super().load_state_dict(sd)
        if buf is not None:
            self.buf.copy_(buf)
        self._hyper_host = None
        self.push_hyper()


class FlatAdam(torch.optim.Optimizer):
    """torch.optim.Adam / AdamW (single-tensor arithmetic, operation for operation) over the flat parameter vector, FlatSGD's sibling:
    it reads the flat gradient bucket, takes the mean inside the update (`grad_scale`), honours the sticky grid-barrier failure words
    and the rank-reduced guard slot, follows an LR scheduler inside a captured graph (``push_hyper()``) and issues no framework kernel:
    two library launches per step (csrc/optim.hip: adam_prologue_kernel, adam_update_kernel), three with `max_grad_norm`.

    The step count ``t`` is a DEVICE word (``opt.t``, int64): the host does not run while a captured step is replayed, so a launch
    scalar would freeze the bias corrections at capture time.  The one-thread prologue launch reads the guard, advances ``t`` -- not
    on a skipped step -- and writes the step's coefficients (both bias corrections in float64 from the betas as Python holds them) for
    the update launch to read; every workgroup of a step therefore sees the same ``t``.  While a failure word or the bucket's guard slot
    is set, ``flat``, ``exp_avg``, ``exp_avg_sq``, ``max_exp_avg_sq`` and ``t`` all stay untouched, in eager steps and replays alike.

    max_grad_norm: global-norm clipping as ``torch.nn.utils.clip_grad_norm_(params, max_grad_norm)`` (norm_type 2,
    error_if_nonfinite=False) in front of the step.  The norm of ``grad_scale * grad`` is a float64 sum folded in a fixed order (equal
    bits run to run) and is left in ``opt.grad_norm`` (device float, unclipped) for logging.  Difference from torch: the gradient bucket
    is NOT rewritten -- the coefficient is applied inside the update, ``bucket.flat`` / ``p.grad`` keep the unclipped gradient.

    Further differences from torch.optim.Adam: every element is updated every step, also a parameter whose ``.grad`` was None (its
    bucket slice is zero: its moments decay and it moves by its old momentum where torch would skip it -- FlatSGD's difference); one
    parameter group, float32 only; ``maximize``, ``foreach``, ``fused``, ``capturable`` and ``differentiable`` are not offered.

    The documented sequence is  zero() -> backward -> allreduce_mean() or pack() -> step();  step() refuses nothing under capture
    (Adam has no special first step)."""

    def __init__(self, bucket, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False, decoupled_weight_decay=False,
                 max_grad_norm=None, check_every=64, grad_scale=1.0):
        if not 0.0 <= lr:
            raise ValueError('Invalid learning rate: %r' % (lr,))
        if not 0.0 <= eps:
            raise ValueError('Invalid epsilon value: %r' % (eps,))
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError('Invalid beta parameter at index 0: %r' % (betas[0],))
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError('Invalid beta parameter at index 1: %r' % (betas[1],))
        if not 0.0 <= weight_decay:
            raise ValueError('Invalid weight_decay value: %r' % (weight_decay,))
        if max_grad_norm is not None and not float(max_grad_norm) >= 0.0:
            raise ValueError('Invalid max_grad_norm: %r' % (max_grad_norm,))
        self.bucket = bucket
        self.flat = _rehome(bucket, type(self).__name__)
        dev = self.flat.device
        self.exp_avg = torch.zeros_like(self.flat)
        self.exp_avg_sq = torch.zeros_like(self.flat)
        self.max_exp_avg_sq = torch.zeros_like(self.flat) if amsgrad else None
        self.t = torch.zeros((), dtype=torch.int64, device=dev)            # device step counter (advanced by the prologue launch)
        self.grad_norm = torch.zeros((), dtype=torch.float32, device=dev)  # unclipped norm of grad_scale * grad (max_grad_norm only)
        self.steps = 0                                                      # eager steps (the check_every cadence)
        self.check_every = int(check_every)
        self.grad_scale = float(grad_scale)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        super().__init__(bucket.params, dict(lr=float(lr), betas=(float(betas[0]), float(betas[1])), eps=float(eps),
                                             weight_decay=float(weight_decay), amsgrad=bool(amsgrad),
                                             decoupled_weight_decay=bool(decoupled_weight_decay)))
        lib = _lib.load()
        self._hyper = torch.zeros(8, dtype=torch.float64, device=dev)
        self._coef = torch.zeros(int(lib.crfconv_adam_coef_floats()), dtype=torch.float32, device=dev)
        self._ws = None
        if self.max_grad_norm is not None:
            self._ws = torch.zeros(int(lib.crfconv_adam_workspace(self.flat.numel())) // 8, dtype=torch.float64, device=dev)
        self._hyper_host = None
        self.push_hyper()

    @property
    def lr(self):
        return self.param_groups[0]['lr']

    @lr.setter
    def lr(self, value):
        self.param_groups[0]['lr'] = float(value)

    def add_param_group(self, group):
        if getattr(self, 'param_groups', None):
            raise _lib.CrfConvError('%s keeps ONE parameter group (one flat vector)' % type(self).__name__)
        super().add_param_group(group)

    def push_hyper(self):
        """Copies {lr, beta1, beta2, eps, weight_decay, grad_scale, max_grad_norm} as float64 to the device block the prologue reads,
        if they changed.  step() does this itself when run eagerly; call it explicitly between replays of a captured step."""
        g = self.param_groups[0]
        cur = (float(g['lr']), float(g['betas'][0]), float(g['betas'][1]), float(g['eps']), float(g['weight_decay']),
               float(self.grad_scale), 0.0 if self.max_grad_norm is None else float(self.max_grad_norm), 0.0)
        if cur != self._hyper_host:
            self._hyper.copy_(torch.tensor(cur, dtype=torch.float64), non_blocking=False)
            self._hyper_host = cur

    def zero_grad(self, set_to_none=True):
        self.bucket.zero()

    @torch.no_grad()
    def step(self, closure=None):
        """Expects the gradients in bucket.flat: ``bucket.allreduce_mean()`` (any world size) or ``bucket.pack()`` puts them there
        after backward."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        g = self.param_groups[0]
        capturing = torch.cuda.is_current_stream_capturing()
        if not capturing:
            self.push_hyper()
        arr, nwords = _guard_words(self.flat.device)         # the guard FlatSGD.step describes: same words, same reduced slot
        clip = self._ws is not None
        _lib.call('crfconv_adam_step', ptr(self.flat), ptr(self.bucket.flat), ptr(self.exp_avg), ptr(self.exp_avg_sq),
                  ptr(self.max_exp_avg_sq), self.flat.numel(), ptr(self._hyper), ptr(self.t), ptr(self._coef), ptr(self.grad_norm),
                  1 if g['decoupled_weight_decay'] else 0, 1 if clip else 0, ptr(self._ws), self._ws.numel() * 8 if clip else 0,
                  arr, nwords, ptr(getattr(self.bucket, 'guard', None)), stream_ptr())
        if not capturing:                                    # (a captured step is counted by the device word alone)
            self.steps += 1
            if self.check_every > 0 and self.steps % self.check_every == 0:
                from . import ops
                ops.check_gridsync(self.flat.device, reduced_flag=getattr(self.bucket, 'guard', None))
        return loss

    # ---- state: the flat vectors as they are, or torch.optim.Adam's per-parameter form
    def state_dict(self):
        sd = super().state_dict()
        sd['flat_exp_avg'] = self.exp_avg.clone()
        sd['flat_exp_avg_sq'] = self.exp_avg_sq.clone()
        sd['flat_max_exp_avg_sq'] = None if self.max_exp_avg_sq is None else self.max_exp_avg_sq.clone()
        sd['flat_t'] = int(self.t)
        sd['flat_steps'] = self.steps
        return sd

    def load_state_dict(self, sd):
        sd = dict(sd)
        m, v, vmax = sd.pop('flat_exp_avg', None), sd.pop('flat_exp_avg_sq', None), sd.pop('flat_max_exp_avg_sq', None)
        t = sd.pop('flat_t', None)
        self.steps = int(sd.pop('flat_steps', self.steps))
        super().load_state_dict(sd)
        with torch.no_grad():
            if m is not None:
                self.exp_avg.copy_(m)
            if v is not None:
                self.exp_avg_sq.copy_(v)
            if self.max_exp_avg_sq is not None and vmax is not None:
                self.max_exp_avg_sq.copy_(vmax)
            if t is not None:
                self.t.fill_(int(t))
        self._hyper_host = None
        self.push_hyper()

    def _views(self, flat):
        out, o = [], 0
        for p in self.bucket.params:
            out.append(flat[o:o + p.numel()].view_as(p))
            o += p.numel()
        return out

    def torch_state_dict(self):
        """The state as ``torch.optim.Adam(model.parameters(), ...).state_dict()`` would hold it after the same steps (per-parameter
        ``step`` / ``exp_avg`` / ``exp_avg_sq`` [/ ``max_exp_avg_sq``], this optimizer's hyper-parameters in the one group): load it
        into a torch.optim.Adam over the same parameters to go on there."""
        g = self.param_groups[0]
        n = len(self.bucket.params)
        twin = torch.optim.Adam([torch.zeros(1)], lr=g['lr'], betas=g['betas'], eps=g['eps'], weight_decay=g['weight_decay'],
                                amsgrad=g['amsgrad'], decoupled_weight_decay=g['decoupled_weight_decay'])
        group = dict(twin.state_dict()['param_groups'][0], params=list(range(n)))
        t = int(self.t)
        state = {}
        if t > 0:
            ms, vs = self._views(self.exp_avg), self._views(self.exp_avg_sq)
            xs = self._views(self.max_exp_avg_sq) if self.max_exp_avg_sq is not None else None
            for i in range(n):
                state[i] = {'step': torch.tensor(float(t), dtype=torch.float32), 'exp_avg': ms[i].clone(), 'exp_avg_sq': vs[i].clone()}
                if xs is not None:
                    state[i]['max_exp_avg_sq'] = xs[i].clone()
        return {'state': state, 'param_groups': [group]}

    def load_torch_state(self, sd):
        """Takes the moments and the step count of a ``torch.optim.Adam`` / ``AdamW`` state dict over the same parameters in the same
        order (hyper-parameters stay this optimizer's own).  An empty state is a fresh optimizer.  Raises ValueError when `step`
        differs between parameters (this optimizer keeps ONE counter), or when a parameter or a needed entry is missing."""
        params = self.bucket.params
        ids = [i for grp in sd['param_groups'] for i in grp['params']]
        if len(ids) != len(params):
            raise ValueError('load_torch_state: %d parameters in the state dict, %d here' % (len(ids), len(params)))
        state = sd['state']
        steps = set(int(float(state[i]['step'])) if i in state else 0 for i in ids)
        if len(steps) != 1:
            raise ValueError('load_torch_state: per-parameter `step` differs (%s); FlatAdam keeps one step count' % sorted(steps))
        t = steps.pop()
        names = ['exp_avg', 'exp_avg_sq'] + (['max_exp_avg_sq'] if self.max_exp_avg_sq is not None else [])
        flats = [self.exp_avg, self.exp_avg_sq] + ([self.max_exp_avg_sq] if self.max_exp_avg_sq is not None else [])
        with torch.no_grad():
            for name, flat in zip(names, flats):
                for i, p, view in zip(ids, params, self._views(flat)):
                    if i not in state:
                        view.zero_()
                        continue
                    if name not in state[i]:
                        raise ValueError('load_torch_state: parameter %d has no %r' % (i, name))
                    src = state[i][name]
                    if tuple(src.shape) != tuple(p.shape):
                        raise ValueError('load_torch_state: %s of parameter %d has shape %s, the parameter %s'
                                         % (name, i, tuple(src.shape), tuple(p.shape)))
                    view.copy_(src)
            self.t.fill_(t)


class FlatAdamW(FlatAdam):
    """FlatAdam with decoupled weight decay (torch.optim.AdamW): ``p *= 1 - lr * weight_decay`` in front of the update."""

    def __init__(self, bucket, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, max_grad_norm=None,
                 check_every=64, grad_scale=1.0):
        super().__init__(bucket, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad,
                         decoupled_weight_decay=True, max_grad_norm=max_grad_norm, check_every=check_every, grad_scale=grad_scale)
