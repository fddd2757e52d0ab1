"""CPU: gpu_util.grad_errors / assert_grads_close, the per-tensor comparison of a whole network's parameter gradients on each tensor's
own scale -- on synthetic dicts (what it must accept and what it must reject, beside what relerr reports for the same input), and on
the oracle itself at the shape of test_config1_shape_eval_and_train_vs_oracle (2 x 2048 points, K = 16, one mean-field step, 50
classes, every level halving): an independent float32 evaluation -- the same oracle with the two clouds swapped, which changes the
order of every sum over the batch -- must pass against the float64 run under the rule the HIP path is held to."""
import numpy as np
import pytest
import torch

import _seeded as S
from gpu_util import assert_grads_check_can_fail, assert_grads_close, grad_errors, oracle_grads, relerr
from oracle import native as onative

TOL = 2e-4
TOP = 0.05                                                  # the largest gradient entry of the synthetic sets (the real net: 0.03 ... 0.08)


def synthetic(small=1e-4, n_zero=0, seed=3):
    """ref64: 'big' (largest entry TOP), 'mid' (1e-2), 'small' (`small`), n_zero tensors of 1e-19; ref32 = ref64 (1 + 1e-7 noise)."""
    r = np.random.default_rng(seed)

    def tensor(shape, peak):
        v = r.uniform(-1.0, 1.0, shape)
        return torch.from_numpy(v * (peak / np.abs(v).max()))
    ref64 = {'big.weight': tensor((32, 16), TOP), 'mid.weight': tensor((64,), 1e-2), 'small.bias': tensor((32,), small)}
    for i in range(n_zero):
        ref64['zero%d.bias' % i] = tensor((8,), 1e-19)
    ref32 = {k: (v * (1.0 + 1e-7 * torch.from_numpy(r.uniform(-1, 1, tuple(v.shape))))).float() for k, v in ref64.items()}
    got = {k: v.clone() for k, v in ref32.items()}
    return got, ref32, ref64


def test_rows_are_on_each_tensors_own_scale():
    got, ref32, ref64 = synthetic()
    rows = {r[0]: r for r in grad_errors(got, ref32, ref64)}
    assert set(rows) == set(ref64)
    for k, (_, e, e32, scale, under) in rows.items():
        assert scale == pytest.approx(float(ref64[k].abs().max())) and not under
        assert e == e32 and 0 < e < 3e-7
    assert len(assert_grads_close(got, ref32, ref64, TOL, 'synthetic')) == 3


def test_zeroed_small_tensor_raises_although_relerr_cannot_see_it():
    got, ref32, ref64 = synthetic()
    got['small.bias'] = torch.zeros_like(got['small.bias'])
    assert relerr(got['small.bias'], ref64['small.bias']) < TOL          # the gap: max|a - b| / max(1, |b|) = 1e-4
    with pytest.raises(AssertionError, match='small.bias'):
        assert_grads_close(got, ref32, ref64, TOL, 'zeroed')


def test_tensor_scaled_by_one_part_in_a_thousand_raises():
    for k in ('big.weight', 'small.bias'):
        got, ref32, ref64 = synthetic()
        got[k] = got[k] * (1.0 + 1e-3)
        with pytest.raises(AssertionError, match=k):
            assert_grads_close(got, ref32, ref64, TOL, 'mis-scaled')


def test_anchor_three_times_the_oracles_error_passes_five_times_raises():
    got, ref32, ref64 = synthetic()
    k = 'mid.weight'
    d = torch.from_numpy(np.random.default_rng(5).uniform(-1, 1, tuple(ref64[k].shape)))
    d = d * (1e-3 * float(ref64[k].abs().max()) / float(d.abs().max()))   # e32 = 1e-3 on the tensor's scale: 4 e32 is above TOL
    ref32[k] = ref64[k] + d                                               # (float64: the multiples below are exact)
    got[k] = ref64[k] + 3.0 * d
    rows = {r[0]: r for r in assert_grads_close(got, ref32, ref64, TOL, 'three times e32')}
    assert rows[k][2] == pytest.approx(1e-3) and rows[k][1] == pytest.approx(3e-3)
    got[k] = ref64[k] + 5.0 * d
    with pytest.raises(AssertionError, match=k):
        assert_grads_close(got, ref32, ref64, TOL, 'five times e32')


def test_under_floor_tensor_noise_passes_and_a_real_value_raises():
    got, ref32, ref64 = synthetic(n_zero=8)
    noise = torch.from_numpy(np.random.default_rng(7).uniform(-1, 1, (8,)))
    noise = noise / noise.abs().max()
    got['zero3.bias'] = (1e-7 * TOP) * noise                # float32 noise where the float64 gradient is 1e-19
    rows = {r[0]: r for r in assert_grads_close(got, ref32, ref64, TOL, 'noise under the floor')}
    assert sum(r[4] for r in rows.values()) == 8 and rows['zero3.bias'][4]
    assert rows['zero3.bias'][3] == pytest.approx(1e-3 * TOP) and rows['zero3.bias'][1] == pytest.approx(1e-4)
    got['zero3.bias'] = (1e-2 * TOP) * noise
    with pytest.raises(AssertionError, match='zero3.bias'):
        assert_grads_close(got, ref32, ref64, TOL, 'a value under the floor')


def test_more_than_sixteen_tensors_under_the_floor_raise():
    got, ref32, ref64 = synthetic(n_zero=16)
    assert_grads_close(got, ref32, ref64, TOL, '16 under the floor')
    got, ref32, ref64 = synthetic(n_zero=17)
    with pytest.raises(AssertionError, match='17 tensors'):
        assert_grads_close(got, ref32, ref64, TOL, '17 under the floor')
    assert_grads_close(got, ref32, ref64, TOL, 'a lower floor', floor=1e-18)


def test_nan_missing_key_and_shape_mismatch_raise():
    got, ref32, ref64 = synthetic()
    got['mid.weight'][5] = float('nan')
    with pytest.raises(AssertionError, match='not finite'):
        assert_grads_close(got, ref32, ref64, TOL, 'nan')
    got, ref32, ref64 = synthetic()
    got['big.weight'][0, 0] = float('inf')
    with pytest.raises(AssertionError, match='not finite'):
        assert_grads_close(got, ref32, ref64, TOL, 'inf')
    got, ref32, ref64 = synthetic()
    del got['small.bias']
    with pytest.raises(AssertionError, match='small.bias'):
        assert_grads_close(got, ref32, ref64, TOL, 'missing in got')
    got, ref32, ref64 = synthetic()
    del ref32['small.bias']
    with pytest.raises(AssertionError, match='small.bias'):
        assert_grads_close(got, ref32, ref64, TOL, 'missing in ref32')
    got, ref32, ref64 = synthetic()
    got['extra.bias'] = torch.zeros(3)
    with pytest.raises(AssertionError, match='extra.bias'):
        assert_grads_close(got, ref32, ref64, TOL, 'one too many')
    got, ref32, ref64 = synthetic()
    got['big.weight'] = got['big.weight'].t().contiguous()
    with pytest.raises(AssertionError, match='shapes'):
        assert_grads_close(got, ref32, ref64, TOL, 'transposed')


def test_self_check_picks_the_smallest_tensor_above_the_floor():
    got, ref32, ref64 = synthetic(n_zero=4)
    assert assert_grads_check_can_fail(got, ref32, ref64, TOL, 'synthetic') == 'small.bias'
    got['big.weight'] = got['big.weight'] * 1.01            # a set that misses already: the rejection must still be the bent tensor's own
    assert assert_grads_check_can_fail(got, ref32, ref64, TOL, 'synthetic, one tensor off') == 'small.bias'
    loose = {k: v + 1.0 for k, v in ref64.items()}          # a float32 reference so far off that the anchor allows anything: nothing is rejected
    with pytest.raises(AssertionError, match='passes the per-tensor comparison'):
        assert_grads_check_can_fail(got, loose, ref64, TOL, 'synthetic, useless anchor')


# ------------------------------------------------------------------ the oracle itself at 2 x 2048, K = 16, T = 1, ratios 2
@pytest.fixture(scope='module')
def oracle_runs():
    """float32, float32 with the clouds swapped, float64: the parameter gradients of one training pass (mean cross entropy, 50 classes,
    the classifier's dropout as a seeded mask), tables from the native kNN checker with seeded subsets."""
    from crfconv_amd import models
    B, N, ncls = 2, 2048, 50
    pos = np.stack([S.make_cloud(40 + b, N) for b in range(B)])
    feats = torch.from_numpy(np.concatenate([pos, S.uniform(40, 'nrm', (B, N, 3))], -1).astype(np.float32))
    labels = torch.from_numpy(S.integers(40, 'y', (B, N), 0, ncls + 1))
    mask = torch.from_numpy(S.integers(40, 'drop', (B, N, 128), 0, 2)).float()
    ms = [{k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in l.items()}
          for l in S.build_multiscale(pos, onative.oracle_knn_batch, ratios=(2,) * 5, seed=40)]
    net = models.PointConvBig(6, ncls, use_crf=True, steps=1)
    sd = S.fill_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, 21)
    was = torch.get_num_threads()
    torch.set_num_threads(16)
    try:
        def run(double, swap):
            f = (lambda v: v.flip(0)) if swap else (lambda v: v)
            return oracle_grads(sd, f(feats), [{k: f(v) for k, v in l.items()} for l in ms], f(labels), 1, double, dropout_mask=f(mask))[2]
        return run(False, False), run(False, True), run(True, False)
    finally:
        torch.set_num_threads(was)


def test_independent_float32_run_of_the_oracle_passes_against_float64(oracle_runs):
    g32, g32_swapped, g64 = oracle_runs
    assert len(g64) == 216
    assert_grads_close(g32_swapped, g32, g64, TOL, 'float32 oracle, clouds swapped')
    assert max(float(v.abs().max()) for v in g64.values()) < 1.0          # relerr's floor of 1 is above every entry of the net


def test_tensors_under_the_floor_are_the_structural_zeros(oracle_runs):
    g32, _, g64 = oracle_runs
    under = sorted(r[0] for r in grad_errors(g32, g32, g64) if r[4])
    assert len(under) <= 16
    zeros = {'deconv%d.%s_nn.1.bn.batch_norm.bias' % (i, w) for i in (1, 2, 3, 4) for w in ('unary', 'pairwise')}
    assert zeros <= set(under), sorted(zeros - set(under))


def test_zeroing_the_smallest_tensor_above_the_floor_raises(oracle_runs):
    g32, g32_swapped, g64 = oracle_runs
    rows = [r for r in grad_errors(g32_swapped, g32, g64) if not r[4]]
    k = min(rows, key=lambda r: r[3])[0]
    bent = dict(g32_swapped)
    bent[k] = torch.zeros_like(bent[k])
    assert relerr(bent[k], g64[k]) < TOL                    # invisible to the old metric
    with pytest.raises(AssertionError, match=k.replace('.', r'\.')):
        assert_grads_close(bent, g32, g64, TOL, 'zeroed ' + k)
    assert assert_grads_check_can_fail(g32_swapped, g32, g64, TOL, 'float32 oracle, clouds swapped') == k
