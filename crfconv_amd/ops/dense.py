"""Per-point Linear and the weight gradient of a plain product, BatchNorm step counters, BatchNorm (+ LeakyReLU)."""

import torch

from .. import _lib
from ..graph import ptr, require_gpu, stream_ptr
from ._base import _f32c, state

# ------------------------------------------------------------------------------ per-point Linear


def _mfma_ok(m, ci, co):
    return m >= state.mfma_min_rows and bool(_lib.load().crfconv_linear_forward_supported(ci, co))


def _gemm(A, B, bias=None, addend=None, nk=False):
    """A [M, K] @ B (+ bias) (+ addend) on the tiled fp32 MFMA kernel of gemm.hip -- the products the row-streaming kernel of
    linear.hip does not take (coarse levels, wide layers; any widths).  nk: B is [N, K] (the F.linear weight), else [K, N].
    Shapes outside the kernel's range (crfconv_gemm_supported: dimensions of 2^24 and more) raise; there is no framework product behind it."""
    M, K = A.shape
    N = B.shape[0] if nk else B.shape[1]
    if M == 0:
        return A.new_empty((0, N))
    if not _lib.load().crfconv_gemm_supported(M, N, K):
        raise _lib.CrfConvError('product %d x %d x %d is outside the tiled kernel\'s range (crfconv_gemm_supported)' % (M, N, K))
    A, B = A.contiguous(), B.contiguous()
    C = torch.empty((M, N), dtype=torch.float32, device=A.device)
    _lib.call('crfconv_gemm', ptr(A), ptr(B), ptr(None if bias is None else bias.contiguous()),
              ptr(None if addend is None else addend.contiguous()), M, N, K, 1 if nk else 0, ptr(C), stream_ptr())
    return C


def _gemm_tn(A, B):
    """A^T B for [m, Ca] / [m, Cb] row operands (a reduction over the long dimension): the MFMA row-reduction kernel of
    wgrad.hip (crfconv_linear_wgrad), fixed summation order."""
    m, ca = A.shape
    cb = B.shape[1]
    if m == 0:
        return A.new_zeros((ca, cb))
    return _wgrad(A.contiguous(), B.contiguous())[0]


def _wgrad(g, x, has_bias=False, out=None):
    """(dW [Co, Ci] = g^T x, db [Co] = the column sums of g, or None) for contiguous [m, Co] / [m, Ci] rows, launched now
    (crfconv_linear_wgrad: partials and their reduction).  out: where dW goes, else a new tensor."""
    m, co = g.shape
    ci = x.shape[1]
    dW = torch.empty((co, ci), dtype=torch.float32, device=g.device) if out is None else out
    db = torch.empty(co, dtype=torch.float32, device=g.device) if has_bias else None
    nbytes = _lib.load().crfconv_linear_wgrad_workspace(m, co, ci)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=g.device)
    _lib.call('crfconv_linear_wgrad', ptr(g), ptr(x), m, co, ci, ptr(dW), ptr(db), ptr(ws), nbytes, stream_ptr())
    return dW, db


def _weight_grad(g, x, params, has_bias):
    """(dW, db) of a plain product y = x W^T (+ b) with params = (W, b): (None, None) where they are left to the batched launches at
    the end of the backward pass (deferred_weight_grads), else computed now."""
    if _defer_ok(params):
        _defer_weight_grad(g, x, params, has_bias)
        return None, None
    return _wgrad(g, x, has_bias)


def _mfma_matmul(x, W, b, transpose_w, want_stats=False):
    """x [m, k] @ (W^T or W) on the fp32 MFMA kernel (linear.hip); optional BatchNorm statistic records."""
    m, ci = x.shape
    co = W.shape[1] if transpose_w else W.shape[0]
    y = torch.empty((m, co), dtype=torch.float32, device=x.device)
    rec = None
    if want_stats:
        nrec = _lib.load().crfconv_linear_forward_stat_records(m)
        rec = torch.empty((nrec, 4, co), dtype=torch.float32, device=x.device)
    _lib.call('crfconv_linear_forward', ptr(x), ptr(W), ptr(b), m, ci, co, 1 if transpose_w else 0, ptr(y), ptr(rec),
              stream_ptr())
    return y, rec


class _Linear(torch.autograd.Function):
    """y = x W^T (+ b) on [m, Ci] rows.  Large-m, <= 128-channel layers run on the MFMA kernels of linear.hip
    and wgrad.hip (forward with fused BatchNorm statistics, dX, and the dW / db row reduction); small or very wide ones go to
    the vendor GEMM for forward / dX (plain library GEMMs)."""

    @staticmethod
    def forward(ctx, x, W, b, want_stats):
        x = x.contiguous()
        Wc = W.contiguous()
        ctx.save_for_backward(x, Wc)
        # the statistic records are a non-differentiable second output: without this autograd zero-fills a gradient
        # for them on every backward call (33 fill launches per training step of PointConvBig)
        ctx.set_materialize_grads(False)
        ctx.has_bias = b is not None
        ctx.params = (W, b)                      # the parameter objects themselves (deferred weight gradients)
        m, ci = x.shape
        rec = None
        if _mfma_ok(m, ci, Wc.shape[0]):
            y, rec = _mfma_matmul(x, Wc, None if b is None else b.contiguous(), False, want_stats)
        else:
            y = _gemm(x, Wc, b, nk=True)
        if want_stats:
            if rec is None:
                rec = torch.empty(0, device=x.device)
            ctx.mark_non_differentiable(rec)
            return y, rec
        return y

    @staticmethod
    def backward(ctx, g, *_unused):
        if g is None:
            return None, None, None, None
        x, W = ctx.saved_tensors
        g = g.contiguous()
        m, Co = g.shape
        Ci = x.shape[1]
        gx = None
        if ctx.needs_input_grad[0]:
            gx = _mfma_matmul(g, W, None, True)[0] if _mfma_ok(m, Co, Ci) else _gemm(g, W)
        dW = db = None
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            dW, db = _weight_grad(g, x, ctx.params, ctx.has_bias)
        return gx, dW, db, None


def linear(x, W, b=None, want_stats=False):
    """Drop-in for F.linear on [..., Ci] CUDA tensors (CPU tensors are refused: there is no CPU path).  With
    want_stats=True returns (y, records) where `records` feeds bn_act(..., records=records) (empty if unused)."""
    require_gpu(x, W)
    if x.dtype != torch.float32 or W.dtype != torch.float32:
        raise _lib.CrfConvError('linear: float32 only (got %s x %s): the path computes in the reference\'s arithmetic' % (x.dtype, W.dtype))
    shape = x.shape
    out = _Linear.apply(x.reshape(-1, shape[-1]), W, b, want_stats)
    if want_stats:
        y, rec = out
        return y.reshape(shape[:-1] + (W.shape[0],)), (rec if rec.numel() else None)
    return out.reshape(shape[:-1] + (W.shape[0],))


# ------------------------------------------------------------------------------ BatchNorm step counters
_COUNTERS_ADVANCED = False


def tick(bn):
    """num_batches_tracked += 1 of one BatchNorm (torch.nn.BatchNorm1d.forward does this in training)."""
    if not _COUNTERS_ADVANCED and bn.num_batches_tracked is not None:
        bn.num_batches_tracked += 1


class advance_counters:
    """``with advance_counters(model):`` around a training forward: the num_batches_tracked buffers of every
    BatchNorm in `model` become views of one int64 vector that advances with a single launch (71 one-element
    launches a step for PointConvBig otherwise).  state_dict keys, shapes and values are unchanged."""

    def __init__(self, module):
        self.module = module

    def __enter__(self):
        global _COUNTERS_ADVANCED
        mod = self.module
        cache = mod.__dict__.get('_bn_counter_cache')
        if cache is None:
            bns = [m for m in mod.modules()
                   if isinstance(m, torch.nn.modules.batchnorm._BatchNorm) and m.num_batches_tracked is not None]
            cache = mod.__dict__['_bn_counter_cache'] = [bns, None]
        bns, flat = cache
        if bns:
            last = bns[-1].num_batches_tracked
            if flat is None or last.device != flat.device or last.data_ptr() != flat[-1].data_ptr():
                flat = cache[1] = torch.stack([b.num_batches_tracked.reshape(()) for b in bns])
                for i, b in enumerate(bns):
                    b._buffers['num_batches_tracked'] = flat[i]
            if flat.is_cuda:
                _lib.call('crfconv_add_i64', ptr(flat), flat.numel(), 1, stream_ptr())
            else:
                flat += 1
        self.prev = _COUNTERS_ADVANCED
        _COUNTERS_ADVANCED = True
        return self

    def __exit__(self, *exc):
        global _COUNTERS_ADVANCED
        _COUNTERS_ADVANCED = self.prev
        return False


# ------------------------------------------------------------------------------ BatchNorm (+ LeakyReLU)
class _BNAct(torch.autograd.Function):
    """y = lrelu(BatchNorm(x), slope) over rows [m, C]: one stats pass + one fused apply pass forward, one
    reduction + one fused pass backward (csrc/bn.hip)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, run_mean, run_var, momentum, eps, use_batch, slope, records):
        m, C = x.shape
        x = x.contiguous()
        y = torch.empty_like(x)
        coef = torch.empty(4 * C, dtype=torch.float32, device=x.device)
        g, b = _f32c(gamma), _f32c(beta)
        if use_batch and records is not None:
            # statistics came out of the Linear kernel's epilogue: no pass over x for them
            _lib.call('crfconv_bn_apply_from_records', ptr(records), records.shape[0], ptr(x), m, C, ptr(g), ptr(b), ptr(run_mean),
                      ptr(run_var), float(momentum), float(eps), None, float(slope), ptr(coef), ptr(y), stream_ptr())
        else:
            nbytes = _lib.load().crfconv_bn_workspace(m, C)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
            _lib.call('crfconv_bn_forward', ptr(x), m, C, ptr(g), ptr(b), ptr(run_mean), ptr(run_var), float(momentum),
                      float(eps), 1 if use_batch else 0, float(slope), ptr(coef), ptr(y), ptr(ws), nbytes, stream_ptr())
        ctx.save_for_backward(x, coef)
        ctx.use_batch, ctx.slope = use_batch, slope
        return y

    @staticmethod
    def backward(ctx, gy):
        x, coef = ctx.saved_tensors
        m, C = x.shape
        gy = gy.contiguous()
        gx = torch.empty_like(x)
        dgamma = torch.empty(C, dtype=torch.float32, device=x.device)
        dbeta = torch.empty(C, dtype=torch.float32, device=x.device)
        nbytes = _lib.load().crfconv_bn_workspace(m, C)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        _lib.call('crfconv_bn_backward', ptr(gy), ptr(x), ptr(coef), m, C, 1 if ctx.use_batch else 0, float(ctx.slope),
                  ptr(gx), ptr(dgamma), ptr(dbeta), ptr(ws), nbytes, stream_ptr())
        return gx, dgamma, dbeta, None, None, None, None, None, None, None


def bn_act(x, bn, training, slope=1.0, records=None):
    """FastBatchNorm1d semantics (statistics over every leading dim of x [..., C]) fused with LeakyReLU(slope);
    `bn` is the torch.nn.BatchNorm1d holding the affine parameters and running statistics.  A channel count that is not a
    multiple of 4 (the kernels' 16-byte granularity; e.g. a 13-class layer) is zero-padded: the pad channels normalise to
    beta = 0 and are cut off again, the running statistics of the real channels are updated in place."""
    shape = x.shape
    C = shape[-1]
    use_batch = training or bn.running_mean is None
    if training:
        tick(bn)
    mom = 0.1 if bn.momentum is None else bn.momentum
    keep_stats = training or not use_batch
    rm, rv = (bn.running_mean, bn.running_var) if keep_stats else (None, None)
    if C % 4:
        Cp = (C + 3) // 4 * 4
        pad = lambda t, v: None if t is None else torch.nn.functional.pad(t, (0, Cp - C), value=v)
        rmp, rvp = pad(rm, 0.0), pad(rv, 1.0)
        y = _BNAct.apply(pad(x.reshape(-1, C), 0.0), pad(bn.weight, 1.0), pad(bn.bias, 0.0), rmp, rvp, mom, bn.eps, use_batch, slope, None)
        if training and rm is not None:
            with torch.no_grad():
                rm.copy_(rmp[:C])
                rv.copy_(rvp[:C])
        return y[:, :C].reshape(shape)
    y = _BNAct.apply(x.reshape(-1, C), bn.weight, bn.bias, rm, rv, mom, bn.eps, use_batch, slope, records)
    return y.reshape(shape)


# ------------------------------------------------------------------------------ inference: the eval-mode MLP block as one launch
def bn_eval_coefs(bns, out=None):
    """(flat, views): the eval-mode coefficient blocks [4, C] = a | b | mean | rstd of the BatchNorm1d modules `bns`, computed from
    their running statistics by ONE launch per 64 modules (crfconv_bn_eval_coef_jobs: what bn_act leaves as `coef` in eval mode,
    the same device code) into one flat float32 device buffer; views[i] is the block of bns[i].  out: a buffer of at least
    4 * sum(C) floats to fill instead of a new one."""
    bns = list(bns)
    if not bns:
        raise _lib.CrfConvError('bn_eval_coefs: no BatchNorm given')
    for bn in bns:
        if not (bn.affine and bn.running_mean is not None and bn.running_var is not None):
            raise _lib.CrfConvError('bn_eval_coefs: affine BatchNorm with running statistics only')
        require_gpu(bn.weight, bn.bias, bn.running_mean, bn.running_var)
        for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var):
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise _lib.CrfConvError('bn_eval_coefs: contiguous float32 parameters and buffers only (got %s)' % t.dtype)
    dev = bns[0].weight.device
    total = 4 * sum(bn.num_features for bn in bns)
    if out is None:
        out = torch.empty(total, dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or out.device != dev or out.numel() < total or not out.is_contiguous():
        raise _lib.CrfConvError('bn_eval_coefs: `out` must be a contiguous float32 buffer of >= %d elements on %s' % (total, dev))
    jobs = (_lib.BnCoefJob * len(bns))()
    views, off = [], 0
    for j, bn in enumerate(bns):
        C = bn.num_features
        view = out[off:off + 4 * C].view(4, C)
        jb = jobs[j]
        jb.gamma, jb.beta, jb.run_mean, jb.run_var = ptr(bn.weight), ptr(bn.bias), ptr(bn.running_mean), ptr(bn.running_var)
        jb.eps, jb.C, jb.coef = float(bn.eps), C, ptr(view)
        views.append(view)
        off += 4 * C
    _lib.call('crfconv_bn_eval_coef_jobs', jobs, len(bns), stream_ptr())
    return out, views


def linear_bn_act(x, W, coef, slope=1.0, skip=None, xb=None, bias=None):
    """lrelu(BN_eval([x | xb] W^T (+ bias)) (+ skip), slope) on [..., Ci] rows as ONE launch: the product kernels with BatchNorm, the
    residual add and the activation in their epilogue (crfconv_linear_bn_act / crfconv_gemm_bn_act).  Inference only -- the result
    has no grad_fn.  coef: the BatchNorm's [4, Co] (or [2, Co]) coefficient block (bn_eval_coefs); slope 1: no activation; skip
    [..., Co]: the ResNet join; xb [..., Cb]: the operand is the column concatenation, left implicit where the row-streaming
    kernel runs and built by cat2 in front of the tiled one.  The kernel is chosen as linear() chooses; the result is
    bit-identical to linear -> bn_act(eval) (-> add_lrelu).  float32 CUDA tensors, Co % 4 == 0."""
    tensors = [t for t in (x, W, coef, skip, xb, bias) if t is not None]
    require_gpu(*tensors)
    for t in tensors:
        if t.dtype != torch.float32:
            raise _lib.CrfConvError('linear_bn_act: float32 only (got %s): the path computes in the reference\'s arithmetic' % t.dtype)
    co = W.shape[0]
    ca = x.shape[-1]
    cb = 0 if xb is None else xb.shape[-1]
    if xb is not None and xb.shape[:-1] != x.shape[:-1]:
        raise _lib.CrfConvError('linear_bn_act: x %s and xb %s differ in their leading shape' % (tuple(x.shape), tuple(xb.shape)))
    if W.dim() != 2 or W.shape[1] != ca + cb:
        raise _lib.CrfConvError('linear_bn_act: W %s does not take %d input channels' % (tuple(W.shape), ca + cb))
    if co % 4:
        raise _lib.CrfConvError('linear_bn_act: %d output channels (a multiple of 4 is needed)' % co)
    if coef.shape[-1] != co or coef.numel() < 2 * co:
        raise _lib.CrfConvError('linear_bn_act: coefficient block %s for %d channels' % (tuple(coef.shape), co))
    if skip is not None and (skip.shape[-1] != co or skip.shape[:-1] != x.shape[:-1]):
        raise _lib.CrfConvError('linear_bn_act: skip %s for an output of %s' % (tuple(skip.shape), tuple(x.shape[:-1]) + (co,)))
    if bias is not None and bias.numel() != co:
        raise _lib.CrfConvError('linear_bn_act: bias of %d elements for %d channels' % (bias.numel(), co))
    from .mlp import cat2
    lead = x.shape[:-1]
    with torch.no_grad():
        x2 = x.detach().reshape(-1, ca).contiguous()
        m = x2.shape[0]
        y = torch.empty((m, co), dtype=torch.float32, device=x.device)
        if m == 0:
            return y.reshape(lead + (co,))
        Wc, cf = W.detach().contiguous(), coef.detach().contiguous()
        b = None if bias is None else bias.detach().contiguous()
        sk = None if skip is None else skip.detach().reshape(-1, co).contiguous()
        xb2 = None if xb is None else xb.detach().reshape(-1, cb).contiguous()
        streaming = _mfma_ok(m, ca + cb, co)
        if xb2 is not None and not (streaming and ca % 4 == 0 and cb % 4 == 0):
            x2, xb2 = cat2(x2, xb2), None
        if streaming:
            _lib.call('crfconv_linear_bn_act', ptr(x2), ptr(xb2), ca if xb2 is not None else 0, ptr(Wc), ptr(b), ptr(cf), ptr(sk),
                      float(slope), m, ca + cb, co, ptr(y), stream_ptr())
        else:
            if not _lib.load().crfconv_gemm_supported(m, co, ca + cb):
                raise _lib.CrfConvError('product %d x %d x %d is outside the tiled kernel\'s range (crfconv_gemm_supported)' % (m, co, ca + cb))
            _lib.call('crfconv_gemm_bn_act', ptr(x2), ptr(Wc), ptr(b), ptr(cf), ptr(sk), float(slope), m, co, ca + cb, 1, ptr(y),
                      stream_ptr())
    return y.reshape(lead + (co,))


def head_eval(x, W1, coef, slope, W2, b2=None):
    """logits [..., C2] = lrelu(BN_eval(x W1^T), slope) W2^T (+ b2) on [..., Ci] rows as ONE launch that never stores the [M, 128]
    activation: the eval form of the classifier head kernel (crfconv_head_forward with a NULL mask; csrc/head.hip), bit-identical
    to that entry point at p = 0 with a mask buffer.  Inference only -- the result has no grad_fn.  coef: the BatchNorm's [4, 128]
    coefficient block a | b | mean | rstd (bn_eval_coefs); the kernel reads a | b.  float32 CUDA tensors; shapes of
    crfconv_head_supported (128 hidden channels, 16 or 32 input channels, at most 16 classes) -- anything else raises."""
    tensors = [t for t in (x, W1, coef, W2, b2) if t is not None]
    require_gpu(*tensors)
    for t in tensors:
        if t.dtype != torch.float32:
            raise _lib.CrfConvError('head_eval: float32 only (got %s): the path computes in the reference\'s arithmetic' % t.dtype)
    ci = x.shape[-1]
    if W1.dim() != 2 or W1.shape[1] != ci:
        raise _lib.CrfConvError('head_eval: W1 %s does not take %d input channels' % (tuple(W1.shape), ci))
    co = W1.shape[0]
    if W2.dim() != 2 or W2.shape[1] != co:
        raise _lib.CrfConvError('head_eval: W2 %s does not take %d hidden channels' % (tuple(W2.shape), co))
    c2 = W2.shape[0]
    if coef.shape[-1] != co or coef.numel() < 2 * co:
        raise _lib.CrfConvError('head_eval: coefficient block %s for %d channels' % (tuple(coef.shape), co))
    if b2 is not None and b2.numel() != c2:
        raise _lib.CrfConvError('head_eval: bias of %d elements for %d classes' % (b2.numel(), c2))
    if not _lib.load().crfconv_head_supported(1, ci, co, c2):
        raise _lib.CrfConvError('head_eval: classifier head %d -> %d -> %d is outside the kernel\'s range (crfconv_head_supported)'
                                % (ci, co, c2))
    lead = x.shape[:-1]
    with torch.no_grad():
        x2 = x.detach().reshape(-1, ci).contiguous()
        m = x2.shape[0]
        logits = torch.empty((m, c2), dtype=torch.float32, device=x.device)
        if m == 0:
            return logits.reshape(lead + (c2,))
        b = None if b2 is None else b2.detach().contiguous()
        _lib.call('crfconv_head_forward', ptr(x2), ptr(W1.detach().contiguous()), ptr(coef.detach().contiguous()), float(slope), 0.0, 0,
                  None, ptr(W2.detach().contiguous()), ptr(b), m, ci, co, c2, ptr(logits), None, None, stream_ptr())
    return logits.reshape(lead + (c2,))


# names of the sibling modules, imported LAST: every use is inside a function body, so import cycles between the families are harmless
from .defer import _defer_ok, _defer_weight_grad  # noqa: E402
