"""-m gpu: the graph builders of models/graph_ops.py on one segmented search per graph.  Every edge list equals, element for element and
in the same order, what the per-cloud loop over knn_batch_device gave (restated here), on a ragged batch with a cloud below k; each
builder makes exactly one crfconv_knn_segments_dev call and no crfconv_knn_batch_dev call."""
import numpy as np
import pytest
import torch

import _seeded as S

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SIZES = [700, 300, 9, 2048, 40]


@pytest.fixture(scope='module')
def batch():
    pos = np.concatenate([S.make_cloud(800 + s, n, box=(2, 1, 1)) + np.float32(3.0 * s) for s, n in enumerate(SIZES)]).astype(np.float32)
    ids = np.repeat(np.arange(len(SIZES)), SIZES).astype(np.int64)
    return torch.from_numpy(pos).to(DEV), torch.from_numpy(ids).to(DEV)


def segments(ids):
    counts = torch.bincount(ids).tolist()
    ends = np.cumsum(counts)
    return [(int(e - c), int(e)) for c, e in zip(counts, ends) if c]


def loop_knn(x, y, k, seg_x, seg_y):
    """The per-cloud loop the builders were: kk = min(k, n) columns for a cloud of n points -> (y_index, x_index)."""
    from crfconv_amd.utils import nearest_neighbors as nn_
    rows, cols = [], []
    for (xs, xe), (ys, ye) in zip(seg_x, seg_y):
        kk = min(k, xe - xs)
        idx = nn_.knn_batch_device(x[xs:xe].unsqueeze(0), y[ys:ye].unsqueeze(0), kk)[0]
        rows.append(torch.arange(ys, ye, device=x.device).unsqueeze(1).expand(-1, kk).reshape(-1))
        cols.append((idx + xs).reshape(-1))
    return torch.cat(rows), torch.cat(cols)


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


def searches(calls, builder):
    """(what `builder()` returns, the kNN library calls it made): a builder is to make exactly one segmented search and no per-cloud one."""
    del calls[:]
    out = builder()
    return out, [c for c in calls if 'knn' in c]


ONE = ['crfconv_knn_segments_dev']


def same(a, b):
    return a.shape == b.shape and np.array_equal(a.cpu().numpy(), b.cpu().numpy())


def test_edge_lists_equal_the_per_cloud_loop(batch, calls):
    from crfconv_amd.models import graph_ops
    pos, ids = batch
    seg = segments(ids)
    k = 16                                                   # above the 9-point cloud: its rows get 9 edges each
    got, made = searches(calls, lambda: graph_ops.knn(pos, pos, k, ids, ids))
    assert made == ONE
    row, col = loop_knn(pos, pos, k, seg, seg)
    assert same(got, torch.stack([row, col])) and got.shape[1] == sum(n * min(k, n) for n in SIZES)

    got, made = searches(calls, lambda: graph_ops.knn_graph(pos, k, ids, loop=True))
    assert made == ONE
    assert same(got, torch.stack([col, row]))

    got, made = searches(calls, lambda: graph_ops.knn_graph(pos, k, ids, loop=False))
    assert made == ONE
    row1, col1 = loop_knn(pos, pos, k + 1, seg, seg)
    keep = row1 != col1
    assert same(got, torch.stack([col1[keep], row1[keep]]))

    r = 0.15
    got, made = searches(calls, lambda: graph_ops.radius_graph(pos, r, ids, loop=False, max_num_neighbors=16))
    assert made == ONE
    keep = (((pos[row1] - pos[col1]) ** 2).sum(1) <= r * r) & (row1 != col1)
    assert same(got, torch.stack([col1[keep], row1[keep]])) and 0 < got.shape[1] < row1.numel()

    got, made = searches(calls, lambda: graph_ops.knn_graph(pos[:700], 8, None, loop=True))       # batch=None: one cloud
    assert made == ONE and same(got, torch.stack(loop_knn(pos[:700], pos[:700], 8, [(0, 700)], [(0, 700)])[::-1]))


def test_fps_and_the_bipartite_search(batch, calls):
    from crfconv_amd.models import graph_ops
    pos, ids = batch
    seg = segments(ids)
    pick = graph_ops.fps(pos, ids, ratio=0.25)
    per_cloud = torch.cat([graph_ops.fps(pos[s:e], None, ratio=0.25) + s for s, e in seg])      # one cloud each: its sorted picks
    assert same(pick, per_cloud) and pick.numel() == sum(-(-n // 4) for n in SIZES)
    sub_pos, sub_ids = pos[pick], ids[pick]
    sub_seg = segments(sub_ids)
    got, made = searches(calls, lambda: graph_ops.knn(sub_pos, pos, 3, sub_ids, ids))      # knn_interpolate's search: 3 subset points for every point
    assert made == ONE
    assert same(got, torch.stack(loop_knn(sub_pos, pos, 3, sub_seg, seg)))
    got, made = searches(calls, lambda: graph_ops.knn(pos, sub_pos, 16, ids, sub_ids))     # build_bipartite_graph's: subset targets gather from the full cloud
    assert made == ONE
    assert same(got, torch.stack(loop_knn(pos, sub_pos, 16, seg, sub_seg)))


def test_dilated_search_keeps_its_draws(batch, calls):
    from crfconv_amd.models import graph_ops
    from crfconv_amd.utils import nearest_neighbors as nn_
    pos, ids = batch
    seg = segments(ids)
    k, d = 6, 3                                              # k d = 18 is above the 9-point cloud
    g1 = torch.Generator(device=DEV).manual_seed(11)
    (row, col), made = searches(calls, lambda: graph_ops.knn_dilated(pos, pos, k, d, ids, ids, generator=g1))
    assert made == ONE
    g2 = torch.Generator(device=DEV).manual_seed(11)
    rows, cols = [], []
    for s, e in seg:                                         # the per-cloud loop it was: search, then randint(have, (n, keep))
        have = min(k * d, e - s)
        idx = nn_.knn_batch_device(pos[s:e].unsqueeze(0), pos[s:e].unsqueeze(0), have)[0]
        keep = min(k, have)
        draw = torch.randint(have, (e - s, keep), dtype=torch.long, device=DEV, generator=g2)
        rows.append(torch.arange(s, e, device=DEV).unsqueeze(1).expand(-1, keep).reshape(-1))
        cols.append((idx.gather(1, draw) + s).reshape(-1))
    assert same(row, torch.cat(rows)) and same(col, torch.cat(cols))


def test_knn_interpolate_on_the_segmented_search(batch, calls):
    """Against a float64 restatement on the same edges.  Features are positive, so the blend has no cancellation and the bound
    is relative to each element: float32 forms d^2, 1 / d^2, the products and two three-term sums, about five roundings of 6e-8."""
    from crfconv_amd import models
    from crfconv_amd.models import graph_ops
    pos, ids = batch
    pick = graph_ops.fps(pos, ids, ratio=0.25)
    sub_pos, sub_ids = pos[pick], ids[pick]
    x = torch.from_numpy(S.uniform(801, 'x', (pick.numel(), 8), 0.5, 1.5)).to(DEV)
    got, made = searches(calls, lambda: models.knn_interpolate(x, sub_pos, pos, sub_ids, ids, k=3))
    assert made == ONE
    row, col = (v.cpu().numpy() for v in graph_ops.knn(sub_pos, pos, 3, sub_ids, ids))
    py, px, xf = pos.cpu().numpy().astype(np.float64), sub_pos.cpu().numpy().astype(np.float64), x.cpu().numpy().astype(np.float64)
    w = 1.0 / np.maximum(((py[row] - px[col]) ** 2).sum(1, keepdims=True), 1e-16)
    num, den = np.zeros((len(py), 8)), np.zeros((len(py), 1))
    np.add.at(num, row, xf[col] * w)
    np.add.at(den, row, w)
    want = num / den
    err = np.abs(got.cpu().numpy() - want) / np.abs(want)
    print('knn_interpolate: max relative error %.3e' % err.max())
    assert err.max() <= 1e-6
