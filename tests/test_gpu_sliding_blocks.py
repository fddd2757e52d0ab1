"""crfconv_amd.blocks.sliding_blocks on the GPU against the NumPy restatement (tests/sliding_blocks_restatement.py), exactly: every
scene of the restatement at the reference's four parameter sets and the tests' own three, a ragged batch against its scenes run alone,
both feature forms bit for bit, take / as_data, two runs bit-identical, a call count that does not grow with the blocks, and the
argument checks.  tests/test_host_sliding_blocks.py holds the conditions on these inputs."""
import numpy as np
import pytest
import torch

import _seeded as S
import sliding_blocks_restatement as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FIELDS = ('ptr', 'indices', 'rows', 'mask', 'batch', 'scene', 'cell', 'pos_min', 'limit')
DTYPES = dict(ptr=torch.int64, indices=torch.int64, rows=torch.int64, mask=torch.int8, batch=torch.int64, scene=torch.int64,
              cell=torch.int32, pos_min=torch.float32, limit=torch.float32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def check_split(got, want, what=''):
    assert (got.n_blocks, got.n_rows) == (want['n_blocks'], want['n_rows']), (what, got.n_blocks, got.n_rows, want['n_blocks'], want['n_rows'])
    for k in FIELDS:
        t = getattr(got, k)
        assert t.is_cuda and t.dtype == DTYPES[k] and tuple(t.shape) == want[k].shape, (what, k, t.dtype, tuple(t.shape), want[k].shape)
        assert np.array_equal(t.cpu().numpy(), want[k]), (what, k)


@pytest.fixture(scope='module')
def scenes():
    """name -> (host points, device points); nothing here is written again."""
    return {name: (p, dev(p)) for name, p in ((name, make()) for name, make in R.SCENES.items())}


@pytest.fixture(scope='module')
def ragged():
    """(host scenes, pos, ptr, device pos, device ptr) of the ragged batch."""
    parts = R.ragged_scenes()
    pos, ptr = np.concatenate(parts), R.ptr_of(parts)
    return parts, pos, ptr, dev(pos), dev(ptr)


@pytest.fixture
def calls(monkeypatch):
    """Names of the library calls made through _lib.call while the fixture is live."""
    from crfconv_amd import _lib
    seen = []
    real = _lib.call

    def call(name, *args):
        seen.append(name)
        return real(name, *args)
    monkeypatch.setattr(_lib, 'call', call)
    return seen


@pytest.mark.parametrize('params', sorted(R.PARAM_SETS))
@pytest.mark.parametrize('scene', sorted(R.SCENES))
def test_split_equals_the_restatement(scenes, scene, params):
    from crfconv_amd import blocks
    p, d = scenes[scene]
    check_split(blocks.sliding_blocks(d, **R.PARAM_SETS[params]), R.np_sliding_blocks(p, **R.PARAM_SETS[params]), (scene, params))


def test_module_parameter_sets_split_like_the_restatement(scenes):
    from crfconv_amd import blocks
    p, d = scenes['carved']
    for name in R.REFERENCE_SETS:
        check_split(blocks.sliding_blocks(d, None, **getattr(blocks, name.upper())), R.np_sliding_blocks(p, **R.REFERENCE_SETS[name]), name)


@pytest.mark.parametrize('params', ['scannet', 'loose', 'semantic3d'])
def test_ragged_batch_equals_the_restatement_and_its_scenes_alone(ragged, params):
    from crfconv_amd import blocks
    parts, pos, ptr, dpos, dptr = ragged
    prm = R.PARAM_SETS[params]
    got = blocks.sliding_blocks(dpos, dptr, **prm)
    check_split(got, R.np_sliding_blocks(pos, ptr, **prm), params)
    b0 = r0 = 0
    host = {k: getattr(got, k).cpu().numpy() for k in FIELDS}
    for s, p in enumerate(parts):
        one = blocks.sliding_blocks(dev(p), dev(np.asarray([0, len(p)], np.int64)), **prm)       # (an empty scene is still one scene)
        nb, nr = one.n_blocks, one.n_rows
        assert (host['scene'][b0:b0 + nb] == s).all()
        assert np.array_equal(host['rows'][r0:r0 + nr], one.rows.cpu().numpy() + ptr[s])
        assert np.array_equal(host['indices'][r0:r0 + nr], one.indices.cpu().numpy())
        assert np.array_equal(host['mask'][r0:r0 + nr], one.mask.cpu().numpy())
        assert np.array_equal(host['batch'][r0:r0 + nr], one.batch.cpu().numpy() + b0)
        assert np.array_equal(host['ptr'][b0:b0 + nb + 1], one.ptr.cpu().numpy() + r0)
        assert np.array_equal(host['cell'][b0:b0 + nb], one.cell.cpu().numpy())
        assert np.array_equal(host['pos_min'][s], one.pos_min.cpu().numpy()[0]) and np.array_equal(host['limit'][s], one.limit.cpu().numpy()[0])
        b0, r0 = b0 + nb, r0 + nr
    assert (b0, r0) == (got.n_blocks, got.n_rows)


def test_a_grid_above_the_first_attempt_is_run_once_more(ragged, calls, monkeypatch):
    from crfconv_amd import blocks
    parts, pos, ptr, dpos, dptr = ragged
    monkeypatch.setattr(blocks, 'CELL_CAP', 7)                       # room for 7 grid cells; the batch has 139
    got = blocks.sliding_blocks(dpos, dptr, **R.LOOSE)
    check_split(got, R.np_sliding_blocks(pos, ptr, **R.LOOSE), 'CELL_CAP = 7')
    assert calls.count('crfconv_sliding_blocks_count') == 2 and calls.count('crfconv_sliding_blocks_emit') == 1


@pytest.mark.parametrize('scene,params', [('planar', 's3dis'), ('carved', 'scannet'), ('yard', 'npm3d'), ('lattice', 'dyadic')])
@pytest.mark.parametrize('form', ['room', 'block'])
@pytest.mark.parametrize('width', [None, 3, 1])
def test_features_equal_the_restatement_bit_for_bit(scenes, scene, params, form, width):
    from crfconv_amd import blocks
    p, d = scenes[scene]
    extra = None if width is None else S.uniform(3340, 'extra', (len(p), width), 0, 1)
    want_split = R.np_sliding_blocks(p, **R.PARAM_SETS[params])
    split = blocks.sliding_blocks(d, **R.PARAM_SETS[params])
    pos_block, x = split.features(form, None if extra is None else dev(extra))
    want_pos, want_x = R.np_features(p, None, want_split, form, extra)
    assert pos_block.dtype == torch.float32 and x.dtype == torch.float32 and x.shape == want_x.shape
    assert np.array_equal(pos_block.cpu().numpy().view(np.uint32), want_pos.view(np.uint32))
    got_x = x.cpu().numpy()
    assert np.array_equal(got_x, want_x, equal_nan=True)
    assert np.array_equal(np.isnan(got_x), np.isnan(want_x)) and np.array_equal(np.signbit(got_x[~np.isnan(got_x)]), np.signbit(want_x[~np.isnan(want_x)]))
    if scene == 'planar' and form == 'room':
        col = (0 if width is None else width) + 2
        assert np.isnan(got_x[:, col]).all()


def test_a_minimum_of_zeros_of_both_signs_is_minus_zero(scenes):
    from crfconv_amd import blocks
    p, d = scenes['zeros']
    want_split = R.np_sliding_blocks(p, **R.S3DIS)
    assert np.signbit(want_split['pos_min'][0]).all() and (want_split['pos_min'][0] == 0).all()
    split = blocks.sliding_blocks(d, **R.S3DIS)
    check_split(split, want_split, 'zeros')
    assert np.array_equal(split.pos_min.cpu().numpy().view(np.uint32), want_split['pos_min'].view(np.uint32))
    for form in ('room', 'block'):
        pos_block, x = split.features(form)
        want_pos, want_x = R.np_features(p, None, want_split, form)
        assert np.array_equal(pos_block.cpu().numpy().view(np.uint32), want_pos.view(np.uint32)), form
        assert np.array_equal(x.cpu().numpy().view(np.uint32), want_x.view(np.uint32)), form
    assert not np.signbit(split.features('room')[0].cpu().numpy()).any()


def test_a_scene_with_too_many_blocks_along_an_axis_is_refused(calls):
    from crfconv_amd import blocks
    far = np.zeros((300, 3), np.float32)
    far[-1] = (3.0e6, 1.0, 0.0)                                      # 6e6 blocks of stride 0.5 along x: above 2^22
    with pytest.raises(ValueError):
        blocks.sliding_blocks(dev(far), **R.S3DIS)
    far[-1] = (1.0e6, 1.0, 0.0)                                      # 2e6 x 1 blocks: allowed, run once more with room for them
    del calls[:]
    got = blocks.sliding_blocks(dev(far), **R.S3DIS)
    assert calls.count('crfconv_sliding_blocks_count') == 2
    assert (got.n_blocks, got.n_rows) == (1, 299) and got.limit.tolist() == [[1.0e6, 1.0, 0.0]]      # the far point's block holds one point
    assert got.rows.tolist() == list(range(299)) and got.cell.tolist() == [[0, 0]] and got.ptr.tolist() == [0, 299]
    assert got.mask.tolist() == [1] * 299 and got.scene.tolist() == [0]


def test_features_of_a_ragged_batch(ragged):
    from crfconv_amd import blocks
    parts, pos, ptr, dpos, dptr = ragged
    extra = S.uniform(3341, 'rgb', (len(pos), 3), 0, 1)
    want_split = R.np_sliding_blocks(pos, ptr, **R.LOOSE)
    split = blocks.sliding_blocks(dpos, dptr, **R.LOOSE)
    for form in ('room', 'block'):
        pos_block, x = split.features(form, dev(extra))
        want_pos, want_x = R.np_features(pos, ptr, want_split, form, extra)
        assert np.array_equal(pos_block.cpu().numpy(), want_pos) and np.array_equal(x.cpu().numpy(), want_x, equal_nan=True), form


def test_take_and_as_data(scenes):
    from crfconv_amd import blocks
    from crfconv_amd.data import Data
    p, d = scenes['carved']
    labels = S.integers(3342, 'y', (len(p),), 0, 20)
    split = blocks.sliding_blocks(d, **R.SCANNET)
    want = R.np_sliding_blocks(p, **R.SCANNET)
    y = split.take(dev(labels))
    assert y.dtype == torch.int64 and np.array_equal(y.cpu().numpy(), labels[want['rows']])
    assert np.array_equal(split.take(d).cpu().numpy(), p[want['rows']])
    pos_block, x = split.features('room')
    data = split.as_data(x, y)
    assert isinstance(data, Data) and sorted(data.keys) == sorted(['pos', 'x', 'y', 'batch', 'ptr', 'mask', 'indices'])
    assert data.pos is pos_block and data.x is x and data.y is y and data.batch is split.batch and data.ptr is split.ptr
    assert data.mask is split.mask and data.indices is split.indices
    assert np.array_equal(data.pos.cpu().numpy(), R.np_features(p, None, want, 'room')[0])
    assert split.as_data(x).y is None
    with pytest.raises(ValueError):
        split.take(dev(labels[:-1]))
    with pytest.raises(ValueError):
        split.as_data(x[:-1])


def test_two_runs_are_bit_identical(ragged):
    from crfconv_amd import blocks
    parts, pos, ptr, dpos, dptr = ragged
    extra = dev(S.uniform(3341, 'rgb', (len(pos), 3), 0, 1))
    runs = []
    for _ in range(2):
        split = blocks.sliding_blocks(dpos, dptr, **R.S3DIS)
        runs.append([getattr(split, k).clone() for k in FIELDS] + list(split.features('block', extra)) + list(split.features('room', extra)))
    for a, b in zip(*runs):
        assert a.dtype == b.dtype and a.shape == b.shape
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)


def test_calls_do_not_grow_with_the_blocks(scenes, ragged, calls):
    from crfconv_amd import blocks
    parts, pos, ptr, dpos, dptr = ragged
    few = blocks.sliding_blocks(scenes['yard'][1], **R.SEMANTIC3D)
    few.features('block')
    n_few, few_calls = few.n_blocks, list(calls)
    del calls[:]
    many = blocks.sliding_blocks(dpos, dptr, **R.LOOSE)
    many.features('block')
    assert many.n_blocks > 10 * n_few and list(calls) == few_calls
    assert few_calls == ['crfconv_sliding_blocks_workspace', 'crfconv_sliding_blocks_count', 'crfconv_sliding_blocks_emit_workspace',
                         'crfconv_sliding_blocks_emit', 'crfconv_sliding_blocks_features']


def test_empty_inputs_and_results(scenes, calls):
    from crfconv_amd import blocks
    none = blocks.sliding_blocks(torch.zeros((0, 3), dtype=torch.float32, device=DEV), **R.SCANNET)
    check_split(none, R.np_sliding_blocks(np.zeros((0, 3), np.float32), np.array([0], np.int64), **R.SCANNET), 'no scene')
    empties = blocks.sliding_blocks(torch.zeros((0, 3), dtype=torch.float32, device=DEV), dev(np.zeros(4, np.int64)), **R.SCANNET)
    check_split(empties, R.np_sliding_blocks(np.zeros((0, 3), np.float32), np.zeros(4, np.int64), **R.SCANNET), 'three empty scenes')
    assert calls == []
    p, d = scenes['tiny']
    split = blocks.sliding_blocks(d, **R.SCANNET)                   # a scene, but no block: no emit launch
    check_split(split, R.np_sliding_blocks(p, **R.SCANNET), 'no block')
    assert 'crfconv_sliding_blocks_emit' not in calls
    pos_block, x = split.features('block', dev(S.uniform(3343, 'e', (len(p), 2), 0, 1)))
    assert tuple(pos_block.shape) == (0, 3) and tuple(x.shape) == (0, 5) and 'crfconv_sliding_blocks_features' not in calls
    assert split.take(d).shape[0] == 0


def test_argument_checks(scenes):
    from crfconv_amd import blocks
    p, d = scenes['tiny']
    n = len(p)
    ok = dict(R.SCANNET)
    with pytest.raises(ValueError):
        blocks.sliding_blocks(d.double(), **ok)
    with pytest.raises(ValueError):
        blocks.sliding_blocks(d[:, :2], **ok)
    with pytest.raises(ValueError):
        blocks.sliding_blocks(d.cpu(), **ok)
    for bad in ([1, n], [0, n - 1], [0, n + 1], [0, 200, 100, n], [0, -1, n]):
        with pytest.raises(ValueError):
            blocks.sliding_blocks(d, dev(np.asarray(bad, np.int64)), **ok)
    with pytest.raises(ValueError):
        blocks.sliding_blocks(d, dev(np.asarray([0, n], np.int32)), **ok)
    for key, value in (('stride', 0.0), ('stride', -1.0), ('block_size', 0.0), ('padding', -0.1), ('count_form', 'floor')):
        with pytest.raises(ValueError):
            blocks.sliding_blocks(d, **dict(ok, **{key: value}))
    with pytest.raises(ValueError):                                  # (ceil(1.0 / 0.125) + 1)^2 = 81 memberships per point
        blocks.sliding_blocks(d, **dict(ok, block_size=1.0, stride=0.125, padding=0.0))
    assert blocks.sliding_blocks(d, **dict(ok, block_size=1.0, stride=0.15, padding=0.0)).n_blocks == 0       # 64: allowed
    split = blocks.sliding_blocks(scenes['carved'][1], **ok)
    with pytest.raises(ValueError):
        split.features('cube')
    with pytest.raises(ValueError):
        split.features('room', scenes['carved'][1][:-1])
    with pytest.raises(ValueError):
        split.features('room', scenes['carved'][1].double())
