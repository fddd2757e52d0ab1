"""-m gpu: farthest point sampling (csrc/fps.hip behind graph_ops.fps / fps_segments) against the float64 restatement of
tests/fps_restatement.py.  Two oracles: the walk-along (every pick is a farthest point within 1e-5, relative) for every cloud, and the
restatement's very picks for the clouds whose every pick is decided by more than that (tests/test_host_fps.py asserts which).  The ragged
batch covers 1, 2, 3, 5 and 8 points per thread, a one-point cloud, a cloud below a wavefront and a size one past a multiple of 1024;
single clouds cover the two larger tiers and the streaming one; a lattice and a repeated point cover ties."""
import numpy as np
import pytest
import torch

import _seeded as S
import fps_restatement as F

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def ptr_of(sizes):
    return dev(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64))


@pytest.fixture(scope='module')
def ragged():
    """(clouds, pos, ptr, ids, the restatement's picks per cloud) of the ragged batch; nothing here is written again."""
    clouds = F.ragged_clouds()
    ids = np.repeat(np.arange(len(F.SIZES)), F.SIZES).astype(np.int64)
    want = [F.np_fps(p, F.n_picks(len(p), F.RATIO))[0] for p in clouds]
    return clouds, dev(np.concatenate(clouds)), ptr_of(F.SIZES), dev(ids), want


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


def check_cloud(p, picks, m, want=None, what=''):
    """picks: the cloud's own rows in pick order."""
    assert len(picks) == m, (what, len(picks), m)
    assert picks.min() >= 0 and picks.max() < len(p), what
    assert len(set(picks.tolist())) == m, what
    worst = F.walk_along(p, picks)
    print('%s: n = %d, %d picks, walk-along worst ratio %.8f%s' % (what, len(p), m, worst, '' if want is None else ', exact'))
    if want is not None:
        assert np.array_equal(picks, want), (what, int(np.argmax(picks != want)))


def test_ragged_batch_in_pick_order(ragged):
    from crfconv_amd.models import graph_ops
    clouds, pos, ptr, ids, want = ragged
    idx, ptr_out = graph_ops.fps_segments(pos, ptr, F.RATIO, sort=False)
    counts = [F.n_picks(n, F.RATIO) for n in F.SIZES]
    assert ptr_out.cpu().tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist() and idx.numel() == sum(counts)
    idx, starts, o = idx.cpu().numpy(), np.concatenate([[0], np.cumsum(F.SIZES)]), 0
    for s, (p, m) in enumerate(zip(clouds, counts)):
        check_cloud(p, idx[o:o + m] - starts[s], m, want[s] if len(p) in F.EXACT else None, 'cloud %d' % s)
        o += m


def test_the_three_forms_agree(ragged):
    from crfconv_amd.models import graph_ops
    clouds, pos, ptr, ids, want = ragged
    by_batch = graph_ops.fps(pos, ids, F.RATIO)                               # the call as it was: positional ratio, batch vector
    by_ptr = graph_ops.fps(pos, ptr=ptr, ratio=F.RATIO)
    seg, ptr_out = graph_ops.fps_segments(pos, ptr, F.RATIO)
    raw, _ = graph_ops.fps_segments(pos, ptr, F.RATIO, sort=False)
    promised = graph_ops.fps(pos, ptr=ptr, ratio=F.RATIO, n_out=by_batch.numel())       # sorted without torch.sort
    assert by_batch.dtype == torch.int64 and torch.equal(by_batch, by_ptr) and torch.equal(by_batch, seg) and torch.equal(by_batch, promised)
    bounds = ptr_out.cpu().tolist()
    assert torch.equal(seg, torch.cat([raw[a:b].sort().values for a, b in zip(bounds[:-1], bounds[1:])]))
    starts = np.concatenate([[0], np.cumsum(F.SIZES)])
    for s, n in enumerate(F.SIZES):                                            # exact clouds: the restatement's picks, sorted
        if n in F.EXACT:
            assert np.array_equal(seg[bounds[s]:bounds[s + 1]].cpu().numpy(), np.sort(want[s]) + starts[s])


def test_batch_equals_each_cloud_alone_and_empty_clouds_get_nothing(ragged):
    from crfconv_amd.models import graph_ops
    clouds, pos, ptr, ids, want = ragged
    raw, _ = graph_ops.fps_segments(pos, ptr, F.RATIO, sort=False)
    bounds = ptr.cpu().tolist()
    alone = [graph_ops.fps_segments(pos[a:b], ptr_of([b - a]), F.RATIO, sort=False)[0] + a for a, b in zip(bounds[:-1], bounds[1:])]
    assert torch.equal(raw, torch.cat(alone))
    assert torch.equal(graph_ops.fps(pos[:700], None, F.RATIO), graph_ops.fps(pos, ids, F.RATIO)[:175])      # batch=None: one cloud
    sizes = [700, 0, 300, 0, 0, 9, 0]                                          # empty clouds in the middle and at the end
    got, ptr_out = graph_ops.fps_segments(pos[:1009], ptr_of(sizes), F.RATIO, sort=False)
    assert (ptr_out[1:] - ptr_out[:-1]).cpu().tolist() == [175, 0, 75, 0, 0, 3, 0]
    assert torch.equal(got, raw[:253])
    none, ptr_out = graph_ops.fps_segments(pos[:0], ptr_of([0, 0]), F.RATIO)
    assert none.numel() == 0 and ptr_out.cpu().tolist() == [0, 0, 0]
    few, _ = graph_ops.fps_segments(pos, ptr, 3, sort=False)                   # an int ratio: min(3, n) picks
    assert few.numel() == sum(min(3, n) for n in F.SIZES)
    assert torch.equal(few[:3], raw[:3]) and torch.equal(few[-3:], raw[raw.numel() - F.n_picks(8192, F.RATIO):][:3])


@pytest.mark.parametrize('seed,n,ratio', F.TIER_CASES)
def test_larger_tiers_make_the_exact_picks(seed, n, ratio):
    from crfconv_amd.models import graph_ops
    p = S.make_cloud(seed, n, box=(2, 1, 1))
    got, _ = graph_ops.fps_segments(dev(p), ptr_of([n]), ratio, sort=False)
    check_cloud(p, got.cpu().numpy(), ratio, F.np_fps(p, ratio)[0], 'tier case')


def test_streaming_tier():
    from crfconv_amd.models import graph_ops
    p = S.make_cloud(952, 65600, box=(2, 1, 1))
    got, _ = graph_ops.fps_segments(dev(p), ptr_of([65600]), 16, sort=False)
    check_cloud(p, got.cpu().numpy(), 16, None, 'streaming')


def test_ties_go_to_the_lower_index():
    from crfconv_amd.models import graph_ops
    lat = (np.stack(np.meshgrid(*[np.arange(8.0)] * 3, indexing='ij'), -1).reshape(-1, 3) * 0.25).astype(np.float32)     # exact in float32
    got, _ = graph_ops.fps_segments(dev(lat), ptr_of([512]), 128, sort=False)
    want, margin = F.np_fps(lat, 128)
    assert margin == 0.0 and np.array_equal(got.cpu().numpy(), want)
    same = np.full((50, 3), 0.7, dtype=np.float32)
    both = dev(np.concatenate([lat, same]))                                    # the repeated point as the second cloud: its row 0 is row 512
    got, _ = graph_ops.fps_segments(both, ptr_of([512, 50]), 13, sort=False)
    assert np.array_equal(got.cpu().numpy(), np.r_[want[:13], [512] * 13])
    assert graph_ops.fps(both, ptr=ptr_of([512, 50]), ratio=13)[13:].cpu().tolist() == [512] * 13
    assert graph_ops.fps(both, ptr=ptr_of([512, 50]), ratio=13, n_out=26)[13:].cpu().tolist() == [512] * 13


def test_random_start(ragged):
    from crfconv_amd.models import graph_ops
    clouds, pos, ptr, ids, want = ragged
    gen = lambda: torch.Generator(device=DEV).manual_seed(21)
    first = graph_ops.random_first(ptr, gen())
    f = first.cpu().numpy()
    assert first.dtype == torch.int64 and (f >= 0).all() and (f < np.array(F.SIZES)).all() and len(set(f[[0, 1, 3, 7, 8]].tolist())) > 1
    raw, ptr_out = graph_ops.fps_segments(pos, ptr, F.RATIO, first=first, sort=False)
    raw, bounds, starts = raw.cpu().numpy(), ptr_out.cpu().tolist(), ptr.cpu().tolist()
    for s, p in enumerate(clouds):
        picks = raw[bounds[s]:bounds[s + 1]] - starts[s]
        assert picks[0] == f[s]
        check_cloud(p, picks, F.n_picks(len(p), F.RATIO), None, 'random start, cloud %d' % s)
    a = graph_ops.fps(pos, ids, F.RATIO, random_start=True, generator=gen())
    b = graph_ops.fps(pos, ids, F.RATIO, True, generator=gen())
    assert torch.equal(a, b) and np.array_equal(a.cpu().numpy(), np.concatenate([np.sort(raw[x:y]) for x, y in zip(bounds[:-1], bounds[1:])]))
    assert graph_ops.fps(pos, ids, F.RATIO, random_start=True).numel() == a.numel()       # the default generator


def test_no_host_work_and_capture(calls):
    """With n_out the call is one library call and can be captured; a replay follows new positions and a new split of the same total."""
    from crfconv_amd.models import graph_ops
    a, b = S.make_cloud(960, 1024, box=(2, 1, 1)), S.make_cloud(961, 1024, box=(1, 2, 1))
    pos, ptr = dev(a).clone(), ptr_of([400, 624])
    del calls[:]
    eager = [t.clone() for t in graph_ops.fps_segments(pos, ptr, F.RATIO, n_out=256)]
    assert calls == ['crfconv_fps']
    assert torch.equal(eager[0], graph_ops.fps_segments(pos, ptr, F.RATIO)[0]) and eager[1].cpu().tolist() == [0, 100, 256]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graph_ops.fps_segments(pos, ptr, F.RATIO, n_out=256, sort=False)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        idx, ptr_out = graph_ops.fps_segments(pos, ptr, F.RATIO, n_out=256)
        raw, _ = graph_ops.fps_segments(pos, ptr, F.RATIO, n_out=256, sort=False)
    for cloud, sizes in ((a, [400, 624]), (b, [400, 624]), (b, [624, 400]), (a, [624, 400])):
        pos.copy_(dev(cloud))
        ptr.copy_(ptr_of(sizes))
        graph.replay()
        want, want_ptr = graph_ops.fps_segments(dev(cloud), ptr_of(sizes), F.RATIO)
        want_raw, _ = graph_ops.fps_segments(dev(cloud), ptr_of(sizes), F.RATIO, sort=False)
        assert torch.equal(idx, want) and torch.equal(ptr_out, want_ptr) and torch.equal(raw, want_raw)
        assert want_ptr.cpu().tolist() == [0, -(-sizes[0] // 4), 256]
    # a promise that does not hold: nothing is written past n_out, and entries past the real total say so
    short, ptr_out = graph_ops.fps_segments(pos, ptr, F.RATIO, n_out=200, sort=False)
    assert torch.equal(short, want_raw[:200]) and ptr_out.cpu().tolist() == [0, 156, 200]
    long, _ = graph_ops.fps_segments(pos, ptr, F.RATIO, n_out=260)
    assert torch.equal(long[:256], want) and long[256:].cpu().tolist() == [1024] * 4


@pytest.mark.parametrize('method', ['knn', 'radius'])
def test_bipartite_builder_on_ptr(ragged, method):
    from crfconv_amd.models import point_conv
    clouds, pos, ptr, ids, want = ragged
    how = dict(method=method, r=0.3, k=16, as_table=True)
    table, sub_pos, sub_batch = point_conv.build_bipartite_graph(pos, ids, F.RATIO, **how)
    for n_out in (None, sub_pos.shape[0]):
        got, got_pos, sub_ptr = point_conv.build_bipartite_graph(pos, None, F.RATIO, ptr=ptr, n_out=n_out, **how)
        assert torch.equal(got.idx32, table.idx32) and got.idx32.shape[0] == sub_pos.shape[0] and int((got.idx32 >= 0).sum()) > 0
        assert torch.equal(got_pos, sub_pos)
        assert torch.equal(sub_ptr[1:] - sub_ptr[:-1], torch.bincount(sub_batch, minlength=len(F.SIZES)))
    with pytest.raises(ValueError):
        point_conv.build_bipartite_graph(pos, ids, F.RATIO, ptr=ptr, **how)
    with pytest.raises(ValueError):
        point_conv.build_bipartite_graph(pos, None, F.RATIO, ptr=ptr, method=method)
