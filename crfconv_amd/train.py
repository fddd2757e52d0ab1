"""The reference training step (trainval.py:99-106) as ONE hipGraph replay, for a caller that keeps its own loop.

    step = CapturedStep(model, optimizer, loss_fn, batch)      # batch: a MultiScaleData that stays resident (static buffers)
    for new_batch in loader:
        loss = step(new_batch)                                 # batch.load_(new_batch) + replay; `loss` is a device scalar

`optimizer` is any torch.optim optimizer whose step() is capturable as is (torch.optim.SGD with float hyper-parameters: a
learning-rate change needs a new CapturedStep) or optim.FlatSGD / optim.FlatAdam (then pass after_backward=bucket.pack).  `loss_fn(logits,
batch)` is the caller's, e.g. ``lambda o, d: F.cross_entropy(o, d.y.reshape(-1) - 1, weight=w, ignore_index=-1)``.
Drop (or detach) losses of earlier EAGER steps of the same model before constructing it: a live loss keeps that step's
autograd nodes -- the parameters' AccumulateGrad nodes, bound to the stream they were created on -- alive, and the capture
would then have to synchronise with that stream.

Round 6: the dense network captures ITSELF (``autograph``).  ``models.PointConvBig`` in training mode hands its forward to a private
GraphedModel (below) the first time it is called on a device batch, so the reference loop with nothing wrapped -- trainval.py:96-106 as
written -- runs as two hipGraph replays per step from its second iteration on.  The other half of that loop -- val_one_epoch and the
test loops, trainval.py:110-124, :170-178, :236-244: ``model.eval()``, then ``model(data)`` under ``no_grad`` -- captures itself too: a private
GraphedInference (at the end of this module) replays the fused eval forward (InferenceNet's launches: logits bit-identical to the
launch-by-launch call) for one batch signature.  What does not fit runs eagerly, silently and correctly -- ``stats(model)`` counts it by reason:
``no_grad`` in training mode (BatchNorm statistics advance there), eval mode with grad enabled (the caller gets a differentiable output),
a batch of other shapes or on another device, a forward whose predecessor has not been through ``backward()`` yet
while anything still reaches that pass's autograd node (a loss is enough -- ``crit(net(b1), y1) + crit(net(b2), y2)``: the replay would
overwrite the activations its backward needs; a pass whose loss was dropped unused no longer counts), module forward / backward hooks on
the model or any submodule and torch's global module hooks (checked at every call, also those registered after the capture), parameters
frozen / thawed since the capture, a call during another stream capture.  Parameters or buffers that are other objects or live at other
addresses than at the capture (``load_state_dict(..., assign=True)``, optim.FlatSGD re-homing them, ``p.data = ...``) drop the graphs;
the model captures again at the first training call that no autograd graph of an earlier pass reaches any more (a loop that releases
its loss before the next forward: at once), eagerly until then; to() / cuda() / float() drop the graphs too.  The logits returned are the caller's own (a copy of the static
output: kept across steps they keep their values).  What raises (RuntimeError) instead of computing something else: the backward of a
replayed pass after a later pass has replayed over its activations, or a second backward of one replayed pass (``retain_graph=True`` does
not keep a replayed pass) -- the model's autograph-off twin gives the eager gradients there.  Still aliased, by design: after
``backward()`` every parameter's ``.grad`` is a view of a static gradient buffer, moved out to storage of its own before the next replay
if still held (accumulation over several backward passes works; a reference kept to an old ``.grad`` object across a zero_grad() and
the next step sees the later values).  ``set_autograph(False)`` / ``CRFCONV_AUTOGRAPH=0`` / ``with no_autograph():`` switch it off (every
launch issued by the host: 2-3 x the step time); ``DistributedDataParallel`` around the model is untested -- switch it off there."""
import collections
import gc
import operator
import os
import weakref

import torch

_AUTO = {'on': os.environ.get('CRFCONV_AUTOGRAPH', '1').strip().lower() not in ('0', 'false', 'off', 'no', ''), 'bypass': 0}


def set_autograph(on):
    """Process-wide switch of the self-capturing training and eval forwards (default on; CRFCONV_AUTOGRAPH=0 starts with it off)."""
    _AUTO['on'] = bool(on)


class no_autograph:
    """``with no_autograph():`` -- models called inside run eagerly (CapturedStep and GraphedModel use it around their own captures)."""

    def __enter__(self):
        _AUTO['bypass'] += 1
        return self

    def __exit__(self, *exc):
        _AUTO['bypass'] -= 1
        return False


def autograph_wanted(batch):
    if not _AUTO['on'] or _AUTO['bypass'] or not torch.is_grad_enabled():
        return False
    return _device_batch(batch) and not torch.cuda.is_current_stream_capturing()


def _device_batch(batch):
    x = getattr(batch, 'x', None)
    return torch.is_tensor(x) and x.is_cuda and hasattr(batch, 'load_') and hasattr(batch, '_apply')


def _eval_refusal(batch):
    """Why an eval-mode call cannot be a replay whatever the runner holds -- one word, or None: grad enabled (the caller gets a
    differentiable output), no device MultiScaleData, a call during another stream capture (issued inline there)."""
    if torch.is_grad_enabled():
        return 'grad'
    if not _device_batch(batch):
        return 'batch'
    if torch.cuda.is_current_stream_capturing():
        return 'capturing'
    return None


def autograph_eval_wanted(batch):
    """The eval-mode twin of autograph_wanted: autograph on and not bypassed, grad DISABLED, a device batch, no capture under way."""
    return bool(_AUTO['on']) and not _AUTO['bypass'] and _eval_refusal(batch) is None


def _stock_network(model):
    """The private eval runner replays InferenceNet's restatement of PointConvResNet._forward: only for a model whose own _forward is
    that one (a subclass that overrides it computes something else) and that InferenceNet takes (decoders all CRF or all Upsampling)."""
    from .infer import why_not
    from .models.point_conv_big import PointConvResNet
    return type(model)._forward is PointConvResNet._forward and why_not(model) is None


def autograph_eval_forward(model, batch):
    """The eval-mode forward of a self-capturing model: the logits of a replay of its private GraphedInference, or None -- the
    model's own forward goes on launch by launch (never a nested ``model(batch)``: the model's hooks fire once).  The runner is
    created by the first call that qualifies; once it exists, calls that do not qualify are counted on it (stats)."""
    if _AUTO['bypass']:
        return None
    runner = model.__dict__.get('_autograph_eval')
    why = 'off' if not _AUTO['on'] else _eval_refusal(batch)
    if why is None and runner is None:
        if _has_hooks(model) or not _stock_network(model):
            return None
        runner = GraphedInference(model)
        object.__setattr__(model, '_autograph_eval', runner)  # (not a submodule of the model: the model is the runner's)
    if why is None:
        why = runner.refusal(batch)
    if why is not None:
        if runner is not None:
            runner.eager[why] += 1
        return None
    return runner.replay(batch)


def count_eager(model, which, why):
    """One more eager call of `model` for the reason `why` on its 'train' / 'eval' runner, if it has one and autograph is on and not
    bypassed (stats: calls inside no_autograph() are not counted; a switched-off call in training mode has no eval reason)."""
    runner = model.__dict__.get('_autograph' if which == 'train' else '_autograph_eval')
    if runner is not None and _AUTO['on'] and not _AUTO['bypass']:
        runner.eager[why] += 1


def stats(model):
    """{'train': {...}, 'eval': {...}} of a self-capturing model (or of a GraphedModel / GraphedInference, under its own key): each
    with `captures`, `replays` and `eager`, a collections.Counter of the calls that ran launch by launch, keyed by a one-word
    reason.  Training runner: 'mode' (eval or no_grad call handed to it), 'hooks', 'pending' (the previous pass still awaits its
    backward), 'passes' (re-homed parameters while an earlier pass's autograd graph lives), 'shape', 'frozen'.  Eval runner: 'off'
    (set_autograph(False)), 'grad', 'training', 'batch', 'dtype', 'capturing', 'hooks', 'phase' (a phase_hook is set: a replay would not
    call it), 'model' (decoders swapped for a mix InferenceNet does not take), 'shape'.  Calls inside ``no_autograph()``
    are not counted.  All zeros for a model that never captured.  Nothing is logged or printed: a loop that degrades from replay
    to launch-by-launch shows here, when asked."""
    runners = {'train': model.__dict__.get('_autograph'), 'eval': model.__dict__.get('_autograph_eval')}
    if isinstance(model, GraphedModel):
        runners['train'] = model
    elif isinstance(model, GraphedInference):
        runners['eval'] = model
    return {k: {'captures': 0 if r is None else r.captures, 'replays': 0 if r is None else r.replays,
                'eager': collections.Counter() if r is None else collections.Counter(r.eager)} for k, r in runners.items()}


def _hook_dicts(modules):
    return [d for m in modules for d in (m._forward_hooks, m._forward_pre_hooks, m._backward_hooks, m._backward_pre_hooks)]


def _global_hooks():
    """torch.nn.modules.module.register_module_forward_hook & co.: they fire for every module, the replayed ones included."""
    M = torch.nn.modules.module
    return bool(M._global_forward_hooks or M._global_forward_pre_hooks or M._global_backward_hooks or M._global_backward_pre_hooks)


def _has_hooks(model):
    return _global_hooks() or any(_hook_dicts(model.modules()))


def autograph_forward(model, batch):
    """The training-mode forward of a self-capturing model: the output of its private GraphedModel, or None -- run eagerly."""
    runner = model.__dict__.get('_autograph')
    if runner is None:
        if _has_hooks(model):
            return None
        runner = GraphedModel(model, guard_pending=True)
        object.__setattr__(model, '_autograph', runner)      # (not a submodule of the model: the model is the runner's)
    elif runner.hooked():
        return None                                          # a hook registered since the capture: the model's own forward calls it
    elif runner.training is not model.training:
        runner.training = model.training                     # (the runner is outside the model's tree: train() / eval() do not reach it)
    return runner(batch)


class CapturedStep:
    def __init__(self, model, optimizer, loss_fn, batch, after_backward=None, warmup=2, defer_weight_grads=True):
        """defer_weight_grads: run the backward inside ``ops.deferred_weight_grads()`` -- the ~150 weight-gradient launches of the
        pass (partial pass + sum per layer) go out as a dozen batched ones at its end; ``.grad`` of every parameter is set before
        ``optimizer.step()`` as usual (same partial slabs, fixed summation order).  False: the backward exactly as the caller wrote it."""
        self.model, self.optimizer, self.loss_fn, self.batch, self.after_backward = model, optimizer, loss_fn, batch, after_backward
        self.defer_weight_grads = bool(defer_weight_grads)
        with no_autograph():                                    # (the model's forward is issued launch by launch inside THIS capture)
            self._build(warmup)

    def _build(self, warmup):
        model, optimizer = self.model, self.optimizer
        # the warm-up steps (allocator, lazily built tables, momentum buffers) must not train: model state is put back afterwards,
        # momentum restarts from zero (mu * 0 + g = g: torch's first step, for dampening = 0)
        import copy
        from .optim import FlatAdam
        flat_adam = isinstance(optimizer, FlatAdam)          # its whole state (moments, device step count) is in its state_dict
        supported = isinstance(optimizer, torch.optim.SGD) or type(optimizer).__name__ == 'FlatSGD' or flat_adam
        if supported and any(float(g.get('dampening', 0.0)) != 0.0 for g in optimizer.param_groups):
            supported = False                                   # (a zeroed momentum buffer gives (1 - d) g, not torch's first step g)
        if not supported and warmup > 0:
            raise TypeError('CapturedStep: the warm-up steps are undone for SGD-type optimizers without dampening (torch.optim.SGD, '
                            'optim.FlatSGD) and for optim.FlatAdam / FlatAdamW only; got %s -- pass warmup=0 and warm the caches up '
                            'yourself' % type(optimizer).__name__)
        keep = [t.detach().clone() for t in list(model.parameters()) + list(model.buffers())]
        opt_state = copy.deepcopy(optimizer.state_dict())       # step counters, schedulers' view of the groups, any other state
        flat_steps = getattr(optimizer, 'steps', None)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(warmup):
                self._step()
            with torch.no_grad():
                for t, k in zip(list(model.parameters()) + list(model.buffers()), keep):
                    t.copy_(k)
                had = bool(opt_state.get('state'))
                if had:
                    optimizer.load_state_dict(opt_state)          # an optimizer that had stepped before: exactly its old state
                for st in optimizer.state.values():
                    if not had and torch.is_tensor(st.get('momentum_buffer')):
                        st['momentum_buffer'].zero_()             # fresh optimizer: mu * 0 + g = g is torch's first step
                if hasattr(optimizer, 'buf'):
                    if 'flat_momentum' in opt_state:
                        optimizer.buf.copy_(opt_state['flat_momentum'])
                    else:
                        optimizer.buf.zero_()
                if flat_steps is not None:
                    optimizer.steps = flat_steps                  # FlatSGD's own counter (its check_every cadence)
                if flat_adam:
                    optimizer.load_state_dict(opt_state)          # moments, amsgrad maximum, device step count t, host counter
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, capture_error_mode='thread_local'):
            self.loss = self._step()

    def _step(self):
        self.optimizer.zero_grad(set_to_none=True)
        loss = self.loss_fn(self.model(self.batch), self.batch)
        if self.defer_weight_grads:
            from . import ops
            with ops.deferred_weight_grads():
                loss.backward()
        else:
            loss.backward()
        if self.after_backward is not None:
            self.after_backward()
        self.optimizer.step()
        return loss.detach()

    def __call__(self, new_batch=None):
        if new_batch is not None:
            self.batch.load_(new_batch)          # into the static buffers; tables, reverse CSRs, moments refreshed in place
        self.graph.replay()
        return self.loss


class _GraphedPass(torch.autograd.Function):
    """model(batch) as one forward replay; the gradient of whatever the caller computed from its output as one backward replay.

    The replays work on ONE set of static buffers: every forward replay overwrites the activations the previous pass saved, and its
    backward replay consumes them (a memory pool shared by both graphs: the backward reuses freed activations for its temporaries).
    `gm._gen` counts both; a pass may run its backward only while the buffers still hold ITS state (ctx.gen == gm._gen) -- a stale or
    repeated backward raises instead of replaying over another pass's activations."""

    @staticmethod
    def forward(ctx, gm, *params):
        gm.fwd_graph.replay()
        gm._gen += 1
        ctx.gm, ctx.gen = gm, gm._gen
        gm._passes.add(ctx)
        if gm.guard_pending:
            # pending until its backward has run or its autograd node is gone (autograph's guard).  The node, not the output: a loss
            # keeps the node alive without keeping the output (cross_entropy saves its own intermediates)
            gm._pending = weakref.ref(ctx)
            return gm.static_out.clone()       # the caller owns its logits: the next replay overwrites static_out
        return gm.static_out.detach()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        gm = ctx.gm
        if ctx.gen != gm._gen:
            raise RuntimeError('crfconv_amd.train: backward through a replayed training pass whose saved activations are gone -- a later '
                               'forward replay overwrote them, or this pass has been through backward() already (retain_graph=True '
                               'does not keep a replayed pass).  Run the backward before the next training call of the model, or run '
                               'this pass eagerly (train.no_autograph()).')
        gm._gen += 1
        gm._pending = None
        gm._keep_accumulated_grads()
        gm.static_gout.copy_(g)
        gm.bwd_graph.replay()
        # fresh tensor objects over the static buffers (as torch.cuda.make_graphed_callables returns them): autograd's AccumulateGrad
        # takes a gradient nobody else holds AS .grad -- handed the objects of gm.static_grads themselves it copies every one of them
        # (about 300 small copy launches per step for PointConvBig, 0.5 ms of the step)
        return (None,) + tuple(None if sg is None else sg.detach() for sg in gm.static_grads)


class _EagerPass(torch.autograd.Function):
    """Identity node behind an output the runner computed eagerly: while it lives (a loss reaches it), so may the parameters' gradient
    accumulators of that pass -- GraphedModel does not capture again then (see forward)."""

    @staticmethod
    def forward(ctx, gm, out):
        gm._passes.add(ctx)
        return out.view_as(out)

    @staticmethod
    def backward(ctx, g):
        return None, g


class GraphedModel(torch.nn.Module):
    """The reference loop UNCHANGED (trainval.py:99-106: zero_grad, model(data), the caller's loss, loss.backward(), optimizer.step())
    at replay cost: wrap the model once,

        net = GraphedModel(models.PointConvBig(6, 13, use_crf=True))       # the loop below it stays as written

    and every training-mode ``net(batch)`` is ONE hipGraph replay of the forward, ``loss.backward()`` ONE replay of the backward
    (the weight-gradient launches batched as in CapturedStep), with the loss and the optimizer the caller's own eager code in
    between -- about 300 library launches per step leave the host as two.  The first training call captures (after `warmup` eager
    passes on a side stream whose effect on BatchNorm statistics and dropout counters is undone); later batches of the SAME shapes
    are copied into the captured batch's buffers (MultiScaleData.load_: one copy launch + the table refreshes).  A batch of other
    shapes, eval mode, no_grad calls, module hooks (any submodule, torch's global ones) and parameters frozen / thawed since the capture
    run the wrapped model eagerly; parameters or buffers re-homed since the capture (other objects or addresses) capture again, once no
    earlier pass's autograd graph is alive (eagerly until then: that graph holds the parameters' gradient accumulators, bound to another stream).  The
    backward of a pass that a later training call has replayed over raises (RuntimeError): without the self-capturing models' pending
    guard (below), ``crit(net(b1)) + crit(net(b2))`` is such a pass.  Parameter gradients come back through autograd (hooks,
    accumulation over several backward passes see ordinary gradients -- tested; a hook-based wrapper such as DistributedDataParallel
    should too, untested); the output -- and, after ``backward()``, every parameter's
    ``.grad`` -- aliases a static buffer that the next call overwrites, as with torch.cuda.make_graphed_callables (gradients still held as ``.grad``
    at the next call are moved out first: _keep_accumulated_grads)."""

    def __init__(self, model, warmup=2, defer_weight_grads=True, guard_pending=False):
        """guard_pending (the self-capturing models' setting): a training call whose predecessor has not been through ``backward()``
        while its autograd node is still reachable runs the model eagerly instead of replaying over it, and the output is a copy of the
        static one (the caller's to keep)."""
        super().__init__()
        self.model = model
        self.warmup, self.defer_weight_grads = int(warmup), bool(defer_weight_grads)
        self.guard_pending, self._pending, self._gen = bool(guard_pending), None, 0
        self._passes = weakref.WeakSet()                         # autograd nodes of this runner's passes that are still alive
        self.captures, self.replays, self.eager = 0, 0, collections.Counter()      # what train.stats reports
        self.fwd_graph = self.bwd_graph = None
        self.static = self.static_out = self.static_gout = None
        self.params, self.static_grads, self._sig = [], [], None
        self._register_state_dict_hook(GraphedModel._strip_prefix_hook.__get__(self))
        self._register_load_state_dict_pre_hook(self._add_prefix_hook)

    # The wrapper is transparent for checkpoints: state_dict keys are the wrapped model's (reference checkpoints load with strict=True,
    # as on the bare model) -- through the module's OWN hooks (the 'model.' prefix is stripped on the way out and put back on the way
    # in), so that a GraphedModel that is a SUBMODULE of something else saves and loads symmetrically too (overriding state_dict /
    # load_state_dict covered the top-level call only: a parent's load recursed past the override and expected 'net.model.<key>').
    def _strip_prefix_hook(self, module, state_dict, prefix, local_metadata):
        inner = prefix + 'model.'
        for k in [k for k in state_dict if k.startswith(inner)]:
            state_dict[prefix + k[len(inner):]] = state_dict.pop(k)
        return state_dict

    def _add_prefix_hook(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        inner = prefix + 'model.'
        for k in [k for k in state_dict if k.startswith(prefix) and not k.startswith(inner)]:
            state_dict[inner + k[len(prefix):]] = state_dict.pop(k)

    def __getattr__(self, name):
        try:
            return super().__getattr__(name)
        except AttributeError:
            return getattr(super().__getattr__('model'), name)

    @staticmethod
    def _signature(batch):
        sig = []

        def visit(t):
            sig.append((tuple(t.shape), t.dtype, t.device))
            return t
        batch._apply(visit)
        return tuple(sig)

    def _backward(self):
        if self.defer_weight_grads:
            from . import ops
            with ops.deferred_weight_grads():
                self.static_out.backward(self.static_gout)
        else:
            self.static_out.backward(self.static_gout)

    def _capture(self, batch):
        self.captures += 1
        # no garbage collection inside the capture: a dead runner of another model (model <-> runner is a reference cycle) owns graphs,
        # and destroying a graph in the middle of another capture aborts the process -- the dead ones go here, before it
        gc.collect()
        was = gc.isenabled()
        gc.disable()
        try:
            with no_autograph():                                # (the wrapped model's forward is issued launch by launch inside this capture)
                self._capture_eagerly_issued(batch)
        finally:
            if was:
                gc.enable()

    def _capture_eagerly_issued(self, batch):
        model = self.model
        self.params = [p for p in model.parameters() if p.requires_grad]
        self.static = batch._apply(torch.clone)
        self._sig = self._signature(batch)
        user_grads = [p.grad for p in self.params]
        keep = [b.detach().clone() for b in model.buffers()]      # BatchNorm statistics, dropout counters: the warm-up must not count
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(max(self.warmup, 1)):                    # (at least one: lazily built tables, allocator, kernel modules)
                for p in self.params:
                    p.grad = None
                self.static_out = model(self.static)
                self.static_gout = torch.zeros_like(self.static_out)
                self._backward()
            with torch.no_grad():
                for b, k in zip(model.buffers(), keep):
                    b.copy_(k)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        for p in self.params:
            p.grad = None
        self.fwd_graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.fwd_graph, capture_error_mode='thread_local'):
            self.static_out = model(self.static)
        self.static_gout = torch.zeros_like(self.static_out)
        self.bwd_graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.bwd_graph, pool=self.fwd_graph.pool(), capture_error_mode='thread_local'):
            self._backward()
        self.static_grads = [p.grad for p in self.params]          # static buffers of the capture pool (None: not reached)
        # the captured autograd graph goes: it holds the parameters' AccumulateGrad nodes, created on the capture's stream, and a
        # node bound to another stream than its caller's costs a stream synchronisation per parameter in every later backward
        self.static_out = self.static_out.detach()
        for p, g in zip(self.params, user_grads):
            p.grad = g
        self._snapshot()                                        # (after the warm-up: the first training forward re-homes the step counters)

    # What the graphs were captured against, kept as flat lists so that the per-call check costs tens of microseconds, not the
    # hundreds of a walk over model.modules() / model.parameters(): every module's hook dictionaries, every module's parameter /
    # buffer / submodule slots (an object put in a slot -- load_state_dict(assign=True), a replaced submodule -- changes an id), the
    # device address of every parameter and buffer (``p.data = ...``, e.g. optim.FlatSGD re-homing the parameters) and requires_grad.
    def _snapshot(self):
        modules = list(self.model.modules())
        self._hooks = _hook_dicts(modules)
        slots = [(d, k, v) for m in modules for d in (m._parameters, m._buffers, m._modules) for k, v in d.items()]
        self._slot_dicts, self._slot_keys, self._slot_objs = [s[0] for s in slots], [s[1] for s in slots], [s[2] for s in slots]
        self._tensors = list(self.model.parameters()) + list(self.model.buffers())
        self._ptrs = list(map(torch.Tensor.data_ptr, self._tensors))
        self._all_params = list(self.model.parameters())
        self._grad_flags = [p.requires_grad for p in self._all_params]

    def hooked(self):
        """A module forward / backward hook on the wrapped model or any submodule, or a global one: the replay would skip it."""
        if self.fwd_graph is None:
            return _has_hooks(self.model)
        return _global_hooks() or any(self._hooks)

    def _moved(self):
        """Parameters or buffers are other objects or live at other addresses than at the capture: the graphs would read stale storage."""
        try:
            same = all(map(operator.is_, map(operator.getitem, self._slot_dicts, self._slot_keys), self._slot_objs))
        except KeyError:                                        # (a slot deleted)
            same = False
        return not same or list(map(torch.Tensor.data_ptr, self._tensors)) != self._ptrs

    def _drop_graphs(self):
        self._gen += 1                                          # (a pass of the old graphs has nothing left to run its backward on)
        self.fwd_graph = self.bwd_graph = None
        self.static = self.static_out = self.static_gout = None
        self.params, self.static_grads, self._sig = [], [], None

    def _keep_accumulated_grads(self):
        """A caller who accumulates over several backward passes (no zero_grad() in between) holds last pass's static buffers as
        ``.grad`` (see _GraphedPass.backward): the next replay -- of the FORWARD already: the two graphs share one memory pool, a
        forward temporary may live where a gradient does -- is about to overwrite them, so they move to storage of their own first.
        The reference loop (zero_grad() every step) finds nothing to move."""
        for p, sg in zip(self.params, self.static_grads):
            if sg is not None and p.grad is not None and p.grad.data_ptr() == sg.data_ptr():
                p.grad = p.grad.clone()

    def _eager(self, batch, why):
        self.eager[why] += 1
        with no_autograph():
            out = self.model(batch)
        return _EagerPass.apply(self, out) if torch.is_tensor(out) and out.requires_grad else out

    def forward(self, batch):
        if not (self.training and torch.is_grad_enabled()):
            return self._eager(batch, 'mode')
        if not self.guard_pending and self.hooked():            # (autograph_forward has checked: the model's own forward runs them)
            return self._eager(batch, 'hooks')
        if self.guard_pending and self._pending is not None:
            if self._pending() is None:
                self._pending = None                            # ... unless its autograd node is gone (a step that skipped its backward)
            else:
                return self._eager(batch, 'pending')            # the previous pass still awaits its backward: nothing may replay over it
        if self.fwd_graph is not None and self._moved():
            self._drop_graphs()                                 # a pending pass of the old graphs raises at its backward (_GraphedPass)
        if self.fwd_graph is None:
            if self._passes:
                # a live autograd graph of an earlier pass holds the parameters' gradient accumulators, bound to the stream they were
                # created on: the captured backward would have to join that stream (the capture fails, or worse) -- eagerly until
                # every earlier pass has been dropped (the next call of a loop that releases its loss before it)
                return self._eager(batch, 'passes')
            self._capture(batch)
        elif batch is not self.static and self._signature(batch) != self._sig:
            return self._eager(batch, 'shape')
        elif [p.requires_grad for p in self._all_params] != self._grad_flags:
            return self._eager(batch, 'frozen')                 # parameters frozen / thawed since the capture
        self._keep_accumulated_grads()
        if batch is not self.static:
            self.static.load_(batch, defer_check=True)          # (no host synchronisation: a bad table raises at the next call)
        self.replays += 1
        return _GraphedPass.apply(self, *self.params)


class GraphedInference:
    """The eval twin of GraphedModel: ``with torch.no_grad(): runner(batch)`` on an eval-mode network as ONE hipGraph replay --
    what val_one_epoch and the test loops of the reference call (trainval.py:110-124, :170-178, :236-244).

        runner = GraphedInference(net)          # net: a PointConvBig (wrapped in a default InferenceNet) or an InferenceNet,
        logits = runner(batch)                  # e.g. InferenceNet(model, fused_head=True); logits [B N, C], the caller's own

    ``models.PointConvBig`` keeps one of its own for its eval-mode calls under ``no_grad`` (autograph_eval_forward), so the
    reference's validation lines need no edit.  The first qualifying call captures (after `warmup` >= 2 eager passes on a side
    stream: a table's first mean-field forward takes another form than its later ones, ops/crf.py), into a memory pool of its own;
    later batches of the SAME shapes are copied into the captured batch's buffers and replayed on the caller's current stream.  ONE
    signature is held.  What runs the network eagerly instead, counted by reason (stats): grad enabled ('grad': the caller gets a
    differentiable output), training mode ('training': BatchNorm statistics advance there), no device MultiScaleData ('batch'),
    features that are not float32 ('dtype'), a call during another stream capture ('capturing': issued inline, as SceneVoter needs
    it), module or global hooks ('hooks'), a set ``phase_hook`` ('phase': the forward calls it, a replay would not), decoders swapped for
    a mix InferenceNet does not take ('model'), other shapes ('shape').  The model's own runner never calls the model again: it
    hands such a call back to the model's forward, so hooks on the model fire once.  Weights and running statistics are read where they live at
    every replay: in-place updates (an optimizer step, load_state_dict) need nothing; parameters or buffers that are other objects
    or sit at other addresses than at the capture drop the graph, and the next call captures again -- at once: there is no
    autograd graph to wait for.  Eval mode mutates no buffer, so the warm-up has nothing to undo."""

    def __init__(self, net, warmup=2):
        from .infer import InferenceNet
        self.target = net                                       # what an eager call runs: the caller's own object
        self.own = not isinstance(net, InferenceNet)            # (our wrapper is outside the model's tree: eval() does not reach it)
        self.net = InferenceNet(net) if self.own else net
        self.model = self.net.model
        self.warmup = max(int(warmup), 2)
        self.captures, self.replays, self.eager = 0, 0, collections.Counter()
        self.graph = self.static = self.static_out = self._sig = None

    _signature = staticmethod(GraphedModel._signature)
    _snapshot = GraphedModel._snapshot                          # slots, addresses and hook dictionaries of self.model
    _moved = GraphedModel._moved

    def hooked(self):
        if self.graph is None:
            return _has_hooks(self.model)
        return _global_hooks() or any(self._hooks)

    def _drop_graph(self):
        self.graph = self.static = self.static_out = self._sig = None

    def _eager(self, batch, why):
        self.eager[why] += 1
        with no_autograph():
            return self.target(batch)

    def _capture(self, batch):
        self.captures += 1
        gc.collect()                                            # (as GraphedModel._capture: no graph may be destroyed inside a capture)
        was = gc.isenabled()
        gc.disable()
        try:
            with no_autograph(), torch.no_grad():
                self.static = batch._apply(torch.clone)
                self._sig = self._signature(batch)
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    for _ in range(self.warmup):                # lazily built tables, the coefficient buffer, the mean field's settled form
                        self.net(self.static)
                torch.cuda.current_stream().wait_stream(side)
                torch.cuda.synchronize()
                self.graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(self.graph, pool=torch.cuda.graph_pool_handle(), capture_error_mode='thread_local'):
                    self.static_out = self.net(self.static)
                self._snapshot()
        except BaseException:
            self._drop_graph()
            raise
        finally:
            if was:
                gc.enable()

    def refusal(self, batch):
        """Why this call cannot be a replay -- one word (the keys of stats()['eval']['eager']) -- or None."""
        if torch.is_grad_enabled():
            return 'grad'
        if self.own:
            self.net.training = self.model.training
        if self.model.training or self.net.training:
            return 'training'
        if not _device_batch(batch):
            return 'batch'
        if batch.x.dtype != torch.float32:
            return 'dtype'
        if torch.cuda.is_current_stream_capturing():
            return 'capturing'
        if self.hooked():
            return 'hooks'
        if self.model.phase_hook is not None:
            return 'phase'                                      # (the forward calls it where a phase begins: a replay would not)
        if self.graph is not None and self._moved():
            self._drop_graph()
        if self.graph is None:
            from .infer import why_not
            if why_not(self.model) is not None:
                return 'model'                                  # decoders swapped since the wrapper was built
        elif batch is not self.static and self._signature(batch) != self._sig:
            return 'shape'
        return None

    def __call__(self, batch):
        why = self.refusal(batch)
        return self.replay(batch) if why is None else self._eager(batch, why)

    def replay(self, batch):
        """The logits of `batch` from one replay (the first one captures); the caller has asked refusal(batch)."""
        if self.graph is None:
            self._capture(batch)
        if batch is not self.static:
            self.static.load_(batch, defer_check=True)          # (no host synchronisation: a bad table raises at the next call)
        self.graph.replay()
        self.replays += 1
        return self.static_out.clone()                          # the caller owns its logits: the next replay overwrites static_out
