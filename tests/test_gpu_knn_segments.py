"""-m gpu: the segmented kNN (crfconv_knn_segments_dev / knn_segments_device) -- one search for a ragged batch of clouds -- against the
per-cloud entry (knn_batch_device on each cloud alone) and the oracle, bit for bit: global ids, -1 fill for clouds with fewer than K
points, empty segments, hostile geometry, non-finite coordinates, hostile pointer arrays, and a captured call replayed over two splits."""
import numpy as np
import pytest
import torch

import _seeded as S
from oracle import native as onative

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module')
def nn_mod():
    from crfconv_amd.utils import nearest_neighbors
    return nearest_neighbors


def dev_ptr(counts):
    return torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)).to(DEV)


def cat(parts):
    return torch.from_numpy(np.concatenate([np.asarray(p, np.float32).reshape(-1, 3) for p in parts])).to(DEV)


def search(nn_mod, pts, qry, K, dtype=torch.int64):
    """The segmented search over lists of per-segment arrays -> [sum nq, K] numpy int64."""
    got = nn_mod.knn_segments_device(cat(pts), dev_ptr([len(p) for p in pts]), cat(qry), dev_ptr([len(q) for q in qry]), K, dtype)
    assert got.dtype == dtype and got.shape == (sum(len(q) for q in qry), K)
    return got.cpu().numpy().astype(np.int64)


def expected(pts, qry, K, knn=onative.oracle_knn):
    """The contract restated per segment with a single-cloud search `knn`: its min(K, n_s) columns plus the segment's first row,
    -1 in the columns a small segment cannot fill, no rows for a segment without queries."""
    rows, first = [], 0
    for p, q in zip(pts, qry):
        want = np.full((len(q), K), -1, np.int64)
        kk = min(K, len(p))
        if kk and len(q):
            want[:, :kk] = knn(np.ascontiguousarray(p, np.float32), np.ascontiguousarray(q, np.float32), kk) + first
        rows.append(want)
        first += len(p)
    return np.concatenate(rows)


# ------------------------------------------------------------------ 1. ragged batch
N_PTS = [1, 2, 17, 700, 64, 5000, 5]
N_QRY = [3, 0, 40, 500, 64, 1000, 9]


@pytest.fixture(scope='module')
def ragged():
    pts, qry = [], []
    for s, (n, m) in enumerate(zip(N_PTS, N_QRY)):
        scale, shift = np.float32(0.5 + 0.75 * s), np.float32(3.0 * s - 4.0)
        box = (1, 1, 1) if s % 2 else (4, 2, 1)
        pts.append(S.make_cloud(300 + s, n, box=box) * scale + shift)
        qry.append((S.make_cloud(350 + s, m, box=box) * np.float32(1.3) - np.float32(0.1)) * scale + shift)     # partly outside the cloud's box
    return pts, qry


@pytest.mark.parametrize('K', [1, 3, 16, 17, 32, 64])
def test_ragged_batch_equals_per_cloud_entry_and_oracle(nn_mod, ragged, K):
    pts, qry = ragged

    def per_cloud(p, q, kk):         # the uniform entry on this cloud alone: whole-cloud search up to 4096 points, the grid above
        return nn_mod.knn_batch_device(torch.from_numpy(p)[None].to(DEV), torch.from_numpy(q)[None].to(DEV), kk)[0].cpu().numpy()
    want = expected(pts, qry, K)
    assert want.shape[0] == sum(N_QRY)                       # the zero-query segment contributes no rows
    assert np.array_equal(want, expected(pts, qry, K, per_cloud))
    for dtype in (torch.int64, torch.int32):
        got = search(nn_mod, pts, qry, K, dtype)
        assert np.array_equal(got, want), (K, dtype, np.argwhere(got != want)[:5])
    small = [s for s, n in enumerate(N_PTS) if n < K]
    assert bool(small) == (K > 1)                            # the -1 fill is exercised for every K above 1


# ------------------------------------------------------------------ 2. ties and hostile geometry
def hostile_cloud(Np, seed):
    """tests/test_gpu_native.py: test_knn_clustered_duplicates_every_search_path's construction, one cloud."""
    rng = np.random.default_rng(seed)
    parts = [rng.normal(0, 0.01, (Np // 4, 3)), rng.normal(2, 0.5, (Np // 4, 3)),
             np.concatenate([rng.uniform(-3, 3, (Np // 4, 2)), np.full((Np // 4, 1), 0.25)], 1)]
    rest = Np - 3 * (Np // 4)
    n_dup = rest // 2
    parts.append(rng.uniform(-4, 4, (rest - n_dup, 3)))
    pts = np.concatenate(parts).astype(np.float32)
    pts = np.concatenate([pts, pts[rng.integers(0, len(pts), n_dup)]])[rng.permutation(Np)]
    assert pts.shape == (Np, 3)
    qry = np.concatenate([pts[: Np // 2], pts[: Np // 4] * np.float32(3.0) + np.float32(7.0)])       # half inside, a quarter far outside
    return pts, np.ascontiguousarray(qry)


@pytest.fixture(scope='module')
def hostile(golden):
    lat = golden('g6_knn.npz')['lattice_pts'].astype(np.float32)
    hp, hq = hostile_cloud(4097, 4097 * 131)
    same = np.tile(np.float32([[0.25, -1.5, 3.0]]), (70, 1))
    same_q = np.concatenate([same[:5], np.float32([[0.0, 0.0, 0.0], [9.0, 9.0, 9.0]])])
    return [lat, hp, same], [lat, hq, same_q]


@pytest.mark.parametrize('K', [16, 17])      # sixteen lanes per query (the dense blob forces pool compactions); one lane per query
def test_ties_and_hostile_geometry_in_one_call(nn_mod, hostile, K):
    pts, qry = hostile
    got = search(nn_mod, pts, qry, K)
    want = expected(pts, qry, K)
    first = 0
    for s, q in enumerate(qry):
        assert np.array_equal(got[first:first + len(q)], want[first:first + len(q)]), (K, 'segment', s)
        first += len(q)


# ------------------------------------------------------------------ 3. edge sizes
def test_edge_sizes_in_one_call(nn_mod):
    K = 16
    sizes = [0, 1, K - 1, K, K + 1]
    pts = [S.make_cloud(400 + s, n) + np.float32(s) for s, n in enumerate(sizes)]
    qry = [S.make_cloud(450 + s, 6) * np.float32(1.5) + np.float32(s) for s in range(len(sizes))]
    for dtype in (torch.int64, torch.int32):
        got = search(nn_mod, pts, qry, K, dtype)
        assert np.array_equal(got, expected(pts, qry, K))
        assert (got[:6] == -1).all()                         # the queries of the empty segment
        assert (got[6:12, 0] == 0).all() and (got[6:12, 1:] == -1).all()
    # nothing but empty segments, and a batch without queries
    assert (search(nn_mod, [np.zeros((0, 3))] * 3, qry[:3], K) == -1).all()
    assert search(nn_mod, pts, [np.zeros((0, 3))] * len(pts), K).shape == (0, K)


# ------------------------------------------------------------------ 4. non-finite coordinates, hostile pointers
@pytest.mark.parametrize('K', [1, 16, 17])
def test_non_finite_coordinates_stay_inside_their_segment(nn_mod, K):
    pts = [S.make_cloud(500 + s, n) * np.float32(2.0) + np.float32(5.0 * s) for s, n in enumerate([300, 400, 50])]
    qry = [S.make_cloud(550 + s, n) * np.float32(2.0) + np.float32(5.0 * s) for s, n in enumerate([64, 100, 20])]
    bad_p, bad_q = pts[1].copy(), qry[1].copy()
    bad_p[[3, 77, 200], [0, 1, 2]] = [np.nan, np.inf, -np.inf]
    bad_p[399] = np.nan
    bad_q[[0, 5, 9, 50], [0, 0, 2, 1]] = [np.nan, np.inf, -np.inf, np.nan]
    bad_q[99] = np.inf
    got = search(nn_mod, [pts[0], bad_p, pts[2]], [qry[0], bad_q, qry[2]], K)          # returning at all is the first property
    mid = got[64:164]
    assert (((mid >= 300) & (mid < 700)) | (mid == -1)).all()
    clean = expected(pts, qry, K)
    assert np.array_equal(got[:64], clean[:64]) and np.array_equal(got[164:], clean[164:])
    # finite queries of the damaged segment still rank its finite points exactly: the non-finite ones are never nearer
    finite_q = np.isfinite(bad_q).all(1)
    finite_p = np.flatnonzero(np.isfinite(bad_p).all(1))
    want = finite_p[onative.oracle_knn(np.ascontiguousarray(bad_p[finite_p]), np.ascontiguousarray(bad_q[finite_q]), K)] + 300
    assert np.array_equal(mid[finite_q], want)


@pytest.mark.parametrize('K', [16, 32])
def test_hostile_pointer_arrays_address_nothing_outside(nn_mod, K):
    """The pointer arrays cannot be validated without a read: the kernels use their running maximum inside [0, total].  Honest segments
    in front of the damage keep their rows; every id is -1 or a row of pts."""
    pts = [S.make_cloud(600 + s, 200) + np.float32(s) for s in range(4)]
    qry = [S.make_cloud(650 + s, 50) + np.float32(s) for s in range(4)]
    P, Q = cat(pts), cat(qry)
    good = expected(pts, qry, K)
    for pp, qp in (([0, 200, 100, 600, 800], [0, 50, 100, 150, 200]),                   # non-monotone
                   ([0, 200, 1 << 40, 5, 800], [0, 50, 100, 150, 200]),                 # far too large, then back
                   ([0, 200, 400, 600, 800], [0, 50, -7, 1 << 33, 3]),                  # damaged query pointers
                   ([-5, -5, -5, -5, -5], [0, 50, 100, 150, 200])):                     # no points at all
        got = nn_mod.knn_segments_device(P, torch.tensor(pp, dtype=torch.int64, device=DEV), Q, torch.tensor(qp, dtype=torch.int64, device=DEV),
                                         K).cpu().numpy()
        assert ((got >= -1) & (got < 800)).all()
        if pp[0] == 0:
            assert np.array_equal(got[:50], good[:50])


# ------------------------------------------------------------------ 5. capture
def test_captured_call_follows_the_pointer_arrays(nn_mod):
    """One captured call, replayed for two splits of the same totals: no size reaches the device through the host."""
    K, total = 16, 4096
    pts = torch.from_numpy(S.make_cloud(700, total, box=(3, 2, 1))).to(DEV)
    qry = torch.from_numpy(S.make_cloud(701, total, box=(3, 2, 1))).to(DEV)
    p_ptr, q_ptr = dev_ptr([total, 0, 0]), dev_ptr([total, 0, 0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        nn_mod.knn_segments_device(pts, p_ptr, qry, q_ptr, K)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = nn_mod.knn_segments_device(pts, p_ptr, qry, q_ptr, K)
    for split in ([3000, 1000, 96], [96, 2000, 2000]):
        assert sum(split) == total
        p_ptr.copy_(dev_ptr(split))
        q_ptr.copy_(dev_ptr(split))
        graph.replay()
        torch.cuda.synchronize()
        got, first = out.cpu().numpy(), 0
        for n in split:
            eager = nn_mod.knn_batch_device(pts[first:first + n][None], qry[first:first + n][None], K)[0] + first
            assert np.array_equal(got[first:first + n], eager.cpu().numpy()), split
            first += n


# ------------------------------------------------------------------ 6. argument errors
def test_argument_errors(nn_mod):
    from crfconv_amd import _lib
    from crfconv_amd._lib import CrfConvError
    from crfconv_amd.graph import ptr, stream_ptr
    pts, qry = torch.zeros(10, 3, device=DEV), torch.zeros(4, 3, device=DEV)
    p_ptr, q_ptr = dev_ptr([10]), dev_ptr([4])
    with pytest.raises(CrfConvError):
        nn_mod.knn_segments_device(torch.zeros(10, 2, device=DEV), p_ptr, torch.zeros(4, 2, device=DEV), q_ptr, 2)      # dim != 3
    for K in (0, 65):
        with pytest.raises(CrfConvError):
            nn_mod.knn_segments_device(pts, p_ptr, qry, q_ptr, K)
    nbytes = _lib.load().crfconv_knn_segments_dev_workspace(1, 10, 4, 2)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    out = torch.empty(4, 2, dtype=torch.int64, device=DEV)
    args = (ptr(pts), ptr(p_ptr), ptr(qry), ptr(q_ptr), 1, 10, 4, 3, 2)
    with pytest.raises(CrfConvError):
        _lib.call('crfconv_knn_segments_dev', *args, None, None, ptr(ws), nbytes, stream_ptr())                       # a null output
    with pytest.raises(CrfConvError):
        _lib.call('crfconv_knn_segments_dev', *args, ptr(out), None, ptr(ws), nbytes - 512, stream_ptr())              # workspace too small
    _lib.call('crfconv_knn_segments_dev', *args, ptr(out), None, ptr(ws), nbytes, stream_ptr())
    assert out.cpu().numpy().tolist() == [[0, 1]] * 4                                                                # ties: the lower id
