"""Helpers shared by the -m gpu parity tests."""
import os

import numpy as np
import torch

DEV = 'cuda'


def t(a, dtype=None, dev=DEV):
    x = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        x = x.to(dtype)
    return x.to(dev)


def relerr(a, b):
    a = a.detach().cpu().double().numpy() if torch.is_tensor(a) else np.asarray(a, dtype=np.float64)
    b = b.detach().cpu().double().numpy() if torch.is_tensor(b) else np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))


# ---- tolerances tied to MEASURED errors (bounds of 1e-4 ... 2e-4 against measured 1e-7 ... 1e-5 leave 100x slack).
# tests/golden/tol_baseline.json holds the LARGEST error the assert_close calls of one (test, `what`) pair measured on an MI355X.
# Re-record after adding / renaming tests or `what` strings (one GPU run, then commit the file):
#     CRFCONV_TOL_RECORD=tests/golden/tol_baseline.json python -m pytest tests -m gpu -q
# Key = pytest node id :: what (round 5: no occurrence counter -- inserting a call no longer shifts the keys behind it).  With the
# baseline present a call must stay within min(its stated bound, TOL_FACTOR x the recorded error), never below the float32 noise
# floor of a normalised comparison: 1e-7, or 16 eps where the recorded run happened to be bit-exact (another summation order, ROCm
# version or GPU moves such a site off zero legitimately).  A call whose key is missing falls back to its stated bound and WARNS
# (new or renamed test, pytest started from another rootdir); CRFCONV_TOL_STRICT=1 turns that into a failure.
_BASELINE_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'tol_baseline.json')
_baseline = None
_recorded = {}
_current = {'node': ''}
_warned = set()
TOL_FACTOR, TOL_FLOOR, TOL_FLOOR_EXACT = 10.0, 1e-7, 16 * 1.1920929e-07


def set_current_test(nodeid):
    _current['node'] = nodeid


def _key(what):
    return '%s::%s' % (_current['node'], what)


def flush_recorded():
    path = os.environ.get('CRFCONV_TOL_RECORD')
    if path and _recorded:
        import json
        with open(path, 'w') as f:
            json.dump(_recorded, f, indent=0, sort_keys=True)


def enforced_bound(key, tol, baseline):
    """(bound, note) for a call with stated bound `tol`: tightened by the recorded error of its key, if there is one."""
    if key not in baseline:
        return tol, None
    rec = float(baseline[key])
    tight = max(TOL_FACTOR * rec, TOL_FLOOR_EXACT if rec == 0.0 else TOL_FLOOR)
    if tight < tol:
        return tight, ' (= max(%g x the error recorded on MI355X, %.3e, noise floor); stated bound %.1e)' % (TOL_FACTOR, rec, tol)
    return tol, ''


def assert_close(a, b, tol, what='', tighten=True):
    """tighten=False: the stated bound only, whatever the baseline recorded -- for comparisons of two TRAJECTORIES (parameters after several
    optimizer steps of two launch sequences that differ in a summation order): their distance is the seed rounding error times whatever the
    steps in between amplify it by, and differs between two runs of the same code on two builds by orders of magnitude (1e-10 ... 1e-6)."""
    global _baseline
    e = relerr(a, b)
    key = _key(what)
    recording = bool(os.environ.get('CRFCONV_TOL_RECORD')) or not tighten
    if os.environ.get('CRFCONV_TOL_RECORD'):
        _recorded[key] = max(_recorded.get(key, 0.0), e)
    if _baseline is None:
        try:
            import json
            _baseline = json.load(open(_BASELINE_PATH))
        except (OSError, ValueError):
            _baseline = {}
    bound, why = (tol, '') if recording else enforced_bound(key, tol, _baseline)
    if why is None:                                       # no recorded error for this call site
        why = ''
        if _baseline and not recording and key not in _warned:
            _warned.add(key)
            msg = 'assert_close: no recorded error for %r in tests/golden/tol_baseline.json -- only the stated bound %.1e is enforced' % (key, tol)
            if os.environ.get('CRFCONV_TOL_STRICT'):
                raise AssertionError(msg + ' (CRFCONV_TOL_STRICT)')
            import warnings
            warnings.warn(msg)
    if os.environ.get('CRFCONV_TEST_REPORT'):             # measured error beside the bound (pytest -s): how much room a bound has
        print('[assert_close] %-44s err %.3e  tol %.1e  enforced %.1e' % (what, e, tol, bound), flush=True)
    assert e <= bound, '%s: max err (rel. to max(1,|ref|)) %.3e > %.1e%s' % (what, e, bound, why)


def load_sd(module, sd_np):
    sd = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd_np.items()}
    module.load_state_dict(sd, strict=True)
    return module


def grads(module):
    return {k: p.grad for k, p in module.named_parameters() if p.grad is not None}


def assert_close_anchored(got, ref32, ref64, tol, what=''):
    """`got` may deviate from the float64 truth by `tol`, or by 4x the CPU float32 oracle's own
    rounding error where that is larger (ill-conditioned sums, e.g. gradients through BatchNorm)."""
    e, e32 = relerr(got, ref64), relerr(ref32, ref64)
    assert e <= max(tol, 4.0 * e32), '%s: err vs fp64 %.3e > max(%.1e, 4 x fp32-oracle err %.3e)' % (what, e, tol, e32)


# ---- parameter gradients of a whole network, each tensor on ITS OWN scale.
# relerr divides by max(1, |ref|): no parameter gradient of a mean cross entropy over 10^4 ... 10^5 points reaches 1 (the largest entry of
# the whole net is below 0.1), so a relerr bound of 2e-4 is an ABSOLUTE one there and cannot see the tensors whose largest entry is below
# it -- a zeroed gradient passes.  grad_errors divides by the tensor's own largest float64 entry instead, floored at `floor` x the largest
# entry of the whole set (`top`): the tensors under that floor are structurally zero (float64 gradient 1e-19, float32 noise 1e-9), where
# no relative figure means anything; assert_grads_close caps how many may be.
def _f64(v):
    return v.detach().cpu().double().numpy() if torch.is_tensor(v) else np.asarray(v, dtype=np.float64)


def _absmax(a):
    return float(np.abs(a).max()) if a.size else 0.0


def grad_errors(got, ref32, ref64, floor=1e-3):
    """One row (name, e, e32, scale, under_floor) per tensor of `ref64`, dicts name -> tensor: e = max|got - ref64| / scale and e32 the
    same of ref32, scale = max(max|ref64_k|, floor x top), top the largest |entry| of all of ref64; differences in float64 on the CPU."""
    r64 = {k: _f64(v) for k, v in ref64.items()}
    top = max([_absmax(v) for v in r64.values()] + [0.0])
    rows = []
    for k, b in r64.items():
        own = _absmax(b)
        scale = max(own, floor * top)
        if scale == 0.0:                                   # (an all-zero reference: any difference is infinitely large)
            scale = float(np.finfo(np.float64).tiny)
        e = _absmax(_f64(got[k]) - b) / scale
        e32 = _absmax(_f64(ref32[k]) - b) / scale
        rows.append((k, e, e32, scale, own < floor * top))
    return rows


def assert_grads_close(got, ref32, ref64, tol, what, floor=1e-3, max_under_floor=16):
    """Every tensor of `got` within max(tol, 4 x the float32 oracle's own error) of the float64 oracle (assert_close_anchored's rule), on the
    tensor's own scale (grad_errors); same keys and shapes in all three, `got` finite, at most `max_under_floor` tensors under the floor.
    Returns the rows.  Sound only where no element of the network sits within rounding of a kink of LeakyReLU or a tie of a max-pool on
    either side: such an element is another function, not another rounding (profiles/r18_gradient_scale.md)."""
    for name, d in (('got', got), ('ref32', ref32)):
        assert set(d) == set(ref64), '%s: %s and ref64 name different tensors: %s' % (what, name, sorted(set(d) ^ set(ref64))[:5])
    for k, b in ref64.items():
        assert tuple(got[k].shape) == tuple(b.shape) == tuple(ref32[k].shape), '%s: %s has shapes %s / %s / %s (got / ref32 / ref64)' % (
            what, k, tuple(got[k].shape), tuple(ref32[k].shape), tuple(b.shape))
        assert np.isfinite(_f64(got[k])).all(), '%s: %s is not finite' % (what, k)
    assert ref64, what
    rows = grad_errors(got, ref32, ref64, floor)
    under = [r[0] for r in rows if r[4]]
    assert len(under) <= max_under_floor, '%s: %d tensors (more than %d) have no entry above %g x the largest gradient entry: %s ...' % (
        what, len(under), max_under_floor, floor, under[:5])
    bad = [r for r in rows if not r[1] <= max(tol, 4.0 * r[2])]
    if bad:
        worst = sorted(rows, key=lambda r: -(r[1] / max(tol, 4.0 * r[2])))[:5]
        raise AssertionError('%s: %d of %d gradient tensors beyond max(%.1e, 4 x fp32-oracle err) of the fp64 oracle on their own scale; worst:\n%s' % (
            what, len(bad), len(rows), tol,
            '\n'.join('  %s: e %.3e  e32 %.3e  scale %.3e  max|ref64| %.3e' % (r[0], r[1], r[2], r[3], _absmax(_f64(ref64[r[0]]))) for r in worst)))
    return rows


def oracle_grads(sd, x, ms, labels, steps, double, dropout_mask=None, class_weights=None, use_crf=True):
    """One training pass of the CPU oracle (trainval.py:99-105) from the state dict `sd`, in float32 or, `double`, in float64 (parameters,
    features, positions, mask and class weights cast; index tables as they are): (logits, loss, {parameter name: gradient})."""
    from oracle import crf_oracle as O

    def cast(v):
        if v is None:
            return None
        v = torch.as_tensor(v).detach().cpu()
        return (v.double() if double else v.clone()) if v.is_floating_point() else v
    prm = {k: cast(v).requires_grad_(v.is_floating_point() and 'running' not in k) for k, v in sd.items()}
    msx = [{k: cast(v) for k, v in l.items()} for l in ms]
    logits = O.pointconv_resnet(prm, cast(x), msx, steps, True, use_crf, dropout_mask=cast(dropout_mask))
    loss = O.training_loss(logits, torch.as_tensor(labels).cpu().long(), cast(class_weights))
    loss.backward()
    return logits.detach(), loss.detach(), {k: v.grad.detach() for k, v in prm.items() if v.requires_grad and v.grad is not None}


def grad_summary(rows, tol):
    """The figures of one site (profiles/r18_gradient_scale.md) from grad_errors' rows."""
    worst = max(rows, key=lambda r: r[1])
    over = [r for r in rows if r[1] > tol]
    ratio = max([r[1] / r[2] if r[2] > 0 else float('inf') for r in over] + [0.0])
    worst32 = max(rows, key=lambda r: r[2])
    return ('tensors %d  under_floor %d  worst e %.3e (%s, e32 %.3e, scale %.3e)  e > %.0e: %d  max e/e32 among them %.2f  |  fp32 oracle alone: '
            'worst e32 %.3e (%s)  e32 > %.0e: %d' % (len(rows), sum(r[4] for r in rows), worst[1], worst[0], worst[2], worst[3], tol, len(over), ratio,
                                                      worst32[2], worst32[0], tol, sum(r[2] > tol for r in rows)))


def assert_grads_check_can_fail(got, ref32, ref64, tol, what, floor=1e-3):
    """The comparison above must reject `got` with its smallest above-floor tensor zeroed, and with that tensor mis-scaled by 10x what the
    rule allows it: arithmetic on results already computed, no launch."""
    rows = [r for r in grad_errors(got, ref32, ref64, floor) if not r[4]]
    k, _, e32, _, _ = min(rows, key=lambda r: r[3])
    for tag, f in (('zeroed', 0.0), ('mis-scaled', 1.0 + 10.0 * max(tol, 4.0 * e32))):
        bent = dict(got)
        bent[k] = got[k].detach().clone() * f
        row = [r for r in grad_errors(bent, ref32, ref64, floor) if r[0] == k][0]
        rejected = not row[1] <= max(tol, 4.0 * row[2])              # by THIS tensor, whatever else `got` may miss
        if rejected:
            try:
                assert_grads_close(bent, ref32, ref64, tol, what, floor)
                rejected = False
            except AssertionError:
                pass
        assert rejected, '%s: %s %s (scale %.3e) passes the per-tensor comparison' % (what, k, tag, row[3])
    return k
