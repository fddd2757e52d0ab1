"""-m gpu: the S3DIS form of the device crop sampler (PossibilitySampler(form='s3dis'), csrc/sampler.hip) and the repeated-index vote
(VoteAccumulator(allow_repeats=True), csrc/evaluate.hip) -- against the fixture the reference's S3DISRoom._get_random produced
(g12_s3dis_sampler.npz), the numpy twins, the eager composition of the collate graph, and today's kernels where the two must agree."""
import numpy as np
import pytest
import torch

import _seeded as S
from gpu_util import DEV, t
from crfconv_amd import transforms as T
from crfconv_amd.sampling import PossibilitySampler, VoteAccumulator, vote_scene
from s3dis_restatement import S3DISTwin, vote_repeated

pytestmark = pytest.mark.gpu
N_DRAWS = 8
FIELDS = ('pos', 'x', 'y', 'point_idx', 'cloud_idx', 'center')


def fixture_sampler(g):
    return PossibilitySampler([t(g['cloud%d' % c]) for c in range(3)], rgb=[t(g['rgb%d' % c]) for c in range(3)],
                              labels=[t(g['labels%d' % c].astype(np.int64)) for c in range(3)], num_points=int(g['num_points']),
                              possibility=[g['poss%d' % c] for c in range(3)], form='s3dis')


def fixture_draws(g):
    k = int(g['num_points'])
    noise = np.stack([g['d%d_noise' % i] for i in range(N_DRAWS)])
    perm = np.full((N_DRAWS, k), -1, np.int64)
    for i in range(N_DRAWS):
        sh = g['d%d_shuffle' % i]
        perm[i, :sh.size] = sh
    choice = np.stack([g['d%d_choice' % i].astype(np.int64) for i in range(N_DRAWS)])
    return noise, perm, choice


def assert_fixture_row(g, i, pos, x, y, point_idx, cloud):
    tag = 'd%d_' % i
    assert int(cloud) == int(g[tag + 'cloud'][0]), i
    assert np.array_equal(point_idx.cpu().numpy(), g[tag + 'point_idx']), i
    assert np.array_equal(pos.cpu().numpy(), g[tag + 'pos']), i
    assert np.array_equal(x.cpu().numpy(), g[tag + 'x']), i
    assert np.array_equal(y.cpu().numpy(), g[tag + 'y']), i


def assert_same_state(a, b):
    for c, (p, q) in enumerate(zip(a.possibility, b.possibility)):
        assert torch.equal(p, q), 'possibility table of cloud %d' % c
    assert torch.equal(a._minv, b._minv) and torch.equal(a._mini, b._mini)


def test_get_random_reproduces_the_reference_fixture(golden):
    g = golden('g12_s3dis_sampler.npz')
    smp = fixture_sampler(g)
    noise, perm, choice = fixture_draws(g)
    k = int(g['num_points'])
    for i in range(N_DRAWS):
        d = smp.get_random(noise=noise[i], perm=perm[i], choice=choice[i])
        assert d.pos.shape == (k, 3) and d.x.shape == (k, 6) and d.y.shape == (k,) and d.point_idx.shape == (k,)
        assert_fixture_row(g, i, d.pos, d.x, d.y, d.point_idx, d.cloud_idx[0])
        assert d.cloud == int(g['d%d_cloud' % i][0])
        assert np.array_equal(smp.min_possibility, g['d%d_min_possibility' % i]), i
    for c in range(3):
        assert np.array_equal(smp.possibility[c].cpu().numpy(), g['possibility%d' % c]), c


@pytest.mark.parametrize('split', [(8,), (3, 5), (1, 1, 2, 4)])
def test_get_batch_reproduces_the_reference_fixture(golden, split):
    """The eight draws as one call and as several consecutive calls (a small room's second visit falls into a later crop of the same call
    or into another call): rows, float64 possibilities and minima bit for bit."""
    g = golden('g12_s3dis_sampler.npz')
    smp = fixture_sampler(g)
    noise, perm, choice = fixture_draws(g)
    at = 0
    for B in split:
        d = smp.get_batch(B, noise=noise[at:at + B], perm=perm[at:at + B], choice=choice[at:at + B])
        for b in range(B):
            assert_fixture_row(g, at + b, d.pos[b], d.x[b], d.y[b], d.point_idx[b], d.cloud_idx[b, 0])
        at += B
        assert np.array_equal(smp.min_possibility, g['d%d_min_possibility' % (at - 1)]), at
    for c in range(3):
        assert np.array_equal(smp.possibility[c].cpu().numpy(), g['possibility%d' % c]), c


def rooms(sizes, seed, box=(6.0, 5.0, 3.0)):
    gen = torch.Generator().manual_seed(seed)
    pts = [(torch.rand(n, 3, generator=gen) * torch.tensor(box)).to(DEV) for n in sizes]
    rgb = [torch.rand(n, 3, generator=gen).to(DEV) for n in sizes]
    labels = [torch.randint(0, 13, (n,), generator=gen).to(DEV) for n in sizes]
    poss = [(torch.randn(n, dtype=torch.float64, generator=gen) * 1e-3) for n in sizes]
    return pts, rgb, labels, poss


def s3dis_pair(sc, k, **kw):
    pts, rgb, labels, poss = sc
    mk = lambda: PossibilitySampler(pts, rgb=rgb, labels=labels, num_points=k, possibility=[p.clone() for p in poss], form='s3dis', **kw)  # noqa: E731
    return mk(), mk()


@pytest.mark.parametrize('sizes,k', [((9000, 2500, 700, 4096), 4096), ((300, 777), 2048), ((70000, 20000, 33000), 40960)])
def test_device_draws_batch_equals_get_random_loop_and_the_numpy_twin(sizes, k):
    """With the device's own draws: get_batch(B) = B get_random calls fed those draws, bit for bit; the draws are the numpy twin's given
    the k_c of each crop; every point of a padded crop appears floor or ceil of k / k_c times."""
    B = 6
    smp, twin = s3dis_pair(rooms(sizes, 31), k, noise_scale=0.35)
    counter = torch.full((1,), 17, dtype=torch.int64, device=DEV)
    batch, noise, perm, choice = smp.get_batch(B, seed=991, counter=counter, return_draws=True)
    assert noise.shape == (B, 3) and perm.shape == (B, k) and choice.shape == (B, k)
    kcs = [min(sizes[int(c)], k) for c in batch.cloud_idx[:, 0]]
    assert any(kc < k for kc in kcs)
    host = PossibilitySampler.draws(991, 17, B, k=k, noise_scale=0.35, kc=kcs)
    assert np.array_equal(perm.cpu().numpy(), host['perm'])
    assert np.array_equal(choice.cpu().numpy(), host['choice'])
    assert np.abs(noise.cpu().numpy() - host['noise']).max() <= 1e-12 * 0.35
    for b in range(B):
        d = twin.get_random(noise=noise[b], perm=perm[b], choice=choice[b])
        assert int(batch.cloud_idx[b, 0]) == int(d.cloud_idx[0]) == d.cloud, b
        for name in ('pos', 'x', 'y', 'point_idx', 'center'):
            assert torch.equal(getattr(batch, name)[b], getattr(d, name)), (b, name)
        mult = torch.bincount(batch.point_idx[b], minlength=sizes[d.cloud])
        mult = mult[mult > 0]
        assert mult.numel() == kcs[b] and int(mult.min()) >= k // kcs[b] and int(mult.max()) <= -(-k // kcs[b]), b
        assert torch.equal(batch.x[b, :, :3], batch.pos[b])
    assert_same_state(smp, twin)
    # the host-drawn path of get_random (generator): shapes and multiplicities only
    d = twin.get_random()
    assert d.pos.shape == (k, 3) and d.x.shape == (k, 6) and d.point_idx.unique().numel() == min(sizes[d.cloud], k)


def test_device_draws_equal_the_numpy_restatement_at_the_edge_shapes():
    """Rooms of 3, 255 and 4097 points at k = 256 (a crop of three rows; one row short of k; a second select tile holding one point),
    the device's own draws: every crop, the final float64 possibility tables and the minima equal S3DISTwin fed those draws, bit for
    bit.  The start possibilities of the two small rooms are lowered by 4e-3 and 2e-3 so that all three rooms are drawn (checked
    beforehand with the restatement on the host: rooms 1, 0, 0, 2, 2, 2; no crop of coincident points, d_max > 0 throughout)."""
    sizes, k, B = (3, 255, 4097), 256, 6
    pts, rgb, labels, poss = rooms(sizes, 63)
    poss = [poss[0] - 4e-3, poss[1] - 2e-3, poss[2]]
    smp, _ = s3dis_pair((pts, rgb, labels, poss), k, noise_scale=0.35)
    twin = S3DISTwin([p.cpu().numpy() for p in pts], [r.cpu().numpy() for r in rgb], [lab.cpu().numpy() for lab in labels],
                     [p.numpy() for p in poss], k)
    counter = torch.full((1,), 17, dtype=torch.int64, device=DEV)
    batch, noise, perm, choice = smp.get_batch(B, seed=991, counter=counter, return_draws=True)
    noise, perm, choice = noise.cpu().numpy(), perm.cpu().numpy(), choice.cpu().numpy()
    kcs, drawn = [], []
    for b in range(B):
        kc = min(sizes[twin.next_cloud()], k)
        ref = twin.draw(noise[b], perm[b, :kc], choice[b])
        assert int(batch.cloud_idx[b, 0]) == ref['cloud'], b
        for name in ('pos', 'x', 'y', 'point_idx'):
            assert np.array_equal(getattr(batch, name)[b].cpu().numpy(), ref[name]), (b, name)
        kcs.append(kc)
        drawn.append(ref['cloud'])
    print('rooms drawn:', drawn)
    assert any(kc < k for kc in kcs) and 2 in drawn
    for c in range(3):
        assert np.array_equal(smp.possibility[c].cpu().numpy(), twin.possibility[c]), c
    assert np.array_equal(smp.min_possibility, np.asarray(twin.min_possibility))


def test_existing_form_is_untouched():
    """form='semantic3d' is the default constructor byte for byte (same seed, same draws), and keeps refusing small clouds."""
    pts, rgb, labels, poss = rooms((20000, 9000), 8, box=(20.0, 20.0, 5.0))
    cw = np.linspace(0.5, 2.0, 13)
    mk = lambda **kw: PossibilitySampler(pts, rgb=rgb, labels=labels, num_points=3000, class_weight=cw,      # noqa: E731
                                         possibility=[p.clone() for p in poss], generator=torch.Generator().manual_seed(5), **kw)
    a, b = mk(), mk(form='semantic3d')
    assert a.form == b.form == 'semantic3d'
    for _ in range(2):
        da, db = a.get_batch(3), b.get_batch(3)
        for name in FIELDS:
            assert torch.equal(getattr(da, name), getattr(db, name)), name
        ra, rb = a.get_random(), b.get_random()
        for name in ('pos', 'rgb', 'y', 'point_idx', 'cloud_idx', 'center'):
            assert torch.equal(getattr(ra, name), getattr(rb, name)), name
    assert_same_state(a, b)
    assert torch.equal(da.pos[..., 2], torch.stack([pts[int(c)][i, 2] for c, i in zip(da.cloud_idx[:, 0], da.point_idx)]))   # z stays raw
    small = rooms((5000, 900), 2)
    smp = PossibilitySampler(small[0], rgb=small[1], labels=small[2], num_points=1000, class_weight=cw, possibility=small[3],
                             form='semantic3d')
    with pytest.raises(ValueError, match='cloud 1'):
        smp.get_batch(2)
    with pytest.raises(ValueError, match='s3dis'):
        smp.get_batch(2, choice=np.zeros((2, 1000), np.int64))


def train_chain():
    return T.Compose([
        T.RandomRotate(degrees=180, axis=2),
        T.RandomScaleAnisotropic(scales=[0.8, 1.2], anisotropic=True),
        T.RandomSymmetry(axis=[True, False, False]),
        T.RandomNoise(sigma=0.001, clip=0.05),
        T.DropFeature(drop_proba=0.2, feature_name='rgb'),
        T.AddFeatsByKeys(list_add_to_x=[True, True], feat_names=['pos', 'rgb'], delete_feats=[False, True]),
    ], generator=torch.Generator().manual_seed(99))


def static_batch(B, N, seed=500):
    import crfconv_amd
    pos = np.stack([S.make_cloud(seed + b, N, box=(2, 2, 1)) for b in range(B)])
    feats = np.concatenate([pos, S.uniform(seed, 'rgb', (B, N, 3), 0, 1)], -1)
    return crfconv_amd.multiscale_compute(t(pos), x=t(feats), y=t(S.integers(seed, 'y', (B, N), 0, 13)),
                                          point_idx=torch.zeros((B, N), dtype=torch.int64, device=DEV),
                                          cloud_idx=torch.zeros((B, 1), dtype=torch.int64, device=DEV),
                                          generator=torch.Generator().manual_seed(1))


def test_collate_graph_over_small_rooms_equals_the_eager_composition():
    """CollateGraph(sampler=<s3dis form, rooms below num_points>, augment=): two replays = get_batch -> augment -> multiscale_compute
    on a twin in the same state, field by field.  A padded crop holds coincident points: the neighbour rows must still be ascending in
    distance and equal a brute-force sort of the distances (the kNN's own float32 arithmetic restated in torch, compared as distances:
    the order among twins is the kNN's tie rule; the augmentation's per-point noise moves twins apart by up to its clip), and
    PointConvBig (eval) on the graph's batch is finite and equals the same network on the eager batch."""
    import crfconv_amd
    from crfconv_amd import models
    from crfconv_amd.data import CollateGraph
    B, N, K = 2, 4096, 16
    chain = train_chain()
    sc = rooms((1500, 3000, 9000), 41)
    sc[3][2] += 4e-3                       # the two small rooms hold the lowest possibilities: the first replay draws both
    smp, twin = s3dis_pair(sc, N)
    static = static_batch(B, N)
    torch.manual_seed(6)
    net = models.PointConvBig(6, 13, True, 3).to(DEV).eval()
    with torch.no_grad():
        net(static)                  # the tables the network derives from the static batch exist before the capture, which refreshes them
    cg = CollateGraph(static, generator=torch.Generator().manual_seed(9), augment=chain, sampler=smp)
    padded = 0
    for i in range(2):
        assert cg.run() is static
        counter = torch.full((1,), i + 1, dtype=torch.int64, device=DEV)
        d = twin.get_batch(B, seed=cg.seed, counter=counter)
        assert_same_state(smp, twin)
        chain.apply_batch(d.pos, d.x, cg.seed, counter)
        order = crfconv_amd.data.morton_order(d.pos)
        assert torch.equal(order, cg.order)
        ref = crfconv_amd.multiscale_compute(d.pos, x=d.x, y=d.y, point_idx=d.point_idx, cloud_idx=d.cloud_idx,
                                             choices=[c.clone() for c in cg.choices], sort='morton', order=order)
        for name in ('x', 'y', 'point_idx', 'cloud_idx'):
            assert torch.equal(getattr(static, name), getattr(ref, name)), (i, name)
        for la, lb in zip(static.multiscale, ref.multiscale):
            for name in ('pos', 'neighbor_idx', 'sub_idx', 'up_idx'):
                u, v = getattr(la, name), getattr(lb, name)
                assert (u is None and v is None) or torch.equal(u, v), (i, name)
        for b in range(B):
            if static.point_idx[b].unique().numel() == N:
                continue
            padded += 1
            pos = static.multiscale[0].pos[b]
            nbr = static.multiscale[0].neighbor_idx[b]

            def sqdist(q, p):          # csrc/knn.hip sqdist_exact: float32 differences, (dx dx + dy dy) + dz dz, every operation rounded once
                sq = (q - p) * (q - p)
                return (sq[..., 0] + sq[..., 1]) + sq[..., 2]
            got = sqdist(pos[:, None, :], pos[nbr])
            assert bool((got[:, 1:] >= got[:, :-1]).all()), (i, b)
            brute = sqdist(pos[:, None, :], pos[None, :, :]).sort(dim=1).values[:, :nbr.shape[1]]
            err = float((got - brute).abs().max())
            print('replay %d crop %d: max |kNN d^2 - brute-force d^2| = %.3e' % (i, b, err))
            assert torch.equal(got, brute), err            # the same float32 arithmetic on both sides: ties may swap indices, not distances
            assert float(got[:, 0].max()) == 0.0                  # column 0 is the point itself (or an exact twin)
        with torch.no_grad():
            a, r = net(static), net(ref)
        assert bool(torch.isfinite(a).all()) and torch.equal(a, r), i
    assert padded >= 2


def test_repeated_vote_equals_numpy_on_the_padded_fixture_crops(golden):
    g = golden('g12_s3dis_sampler.npz')
    C, smooth = 13, 0.95
    sizes = [g['cloud%d' % c].shape[0] for c in range(3)]
    rng = np.random.default_rng(12)
    runs = []
    for run in range(2):
        votes = VoteAccumulator(sizes, C, smooth=smooth, device=DEV, track_visits=True, allow_repeats=True)
        ref = [np.zeros((n, C), np.float32) for n in sizes]
        ref_visits = [np.zeros(n, np.int32) for n in sizes]
        rng = np.random.default_rng(12)
        repeats = 0
        for i in range(N_DRAWS):
            c = int(g['d%d_cloud' % i][0])
            idx = g['d%d_point_idx' % i].astype(np.int64)
            repeats += idx.size - np.unique(idx).size
            p = rng.random((idx.size, C)).astype(np.float32)
            p /= p.sum(1, keepdims=True)
            votes.update(t(idx).reshape(1, -1), [c], probs=t(p))
            vote_repeated(ref[c], ref_visits[c], idx, p, smooth)
        votes.check()
        assert repeats > 2000
        for c in range(3):
            assert np.array_equal(votes.test_probs[c].cpu().numpy(), ref[c]), c
            assert np.array_equal(votes.visits[c].cpu().numpy(), ref_visits[c]), c
            assert bool((votes._last[c] == -1).all())
        runs.append([tp.clone() for tp in votes.test_probs])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


@pytest.mark.parametrize('use_logits', [False, True])
def test_repeated_vote_on_distinct_rows_equals_todays_kernel(use_logits):
    n, C, k = 5000, 8, 1500
    rng = np.random.default_rng(4)
    old = VoteAccumulator([n], C, device=DEV, track_visits=True)
    new = VoteAccumulator([n], C, device=DEV, track_visits=True, allow_repeats=True)
    for _ in range(5):
        idx = t(rng.choice(n, k, replace=False)).reshape(1, -1)
        src = t(rng.standard_normal((k, C)).astype(np.float32))
        if not use_logits:
            src = torch.softmax(src, 1)
        kw = {'logits': src} if use_logits else {'probs': src}
        old.update(idx, [0], **kw)
        new.update(idx, [0], **kw)
    assert torch.equal(old.test_probs[0], new.test_probs[0]) and torch.equal(old.visits[0], new.visits[0])
    # repeated=False on an accumulator built for repeats is today's path
    idx = t(rng.choice(n, k, replace=False)).reshape(1, -1)
    src = torch.softmax(t(rng.standard_normal((k, C)).astype(np.float32)), 1)
    old.update(idx, [0], probs=src)
    new.update(idx, [0], probs=src, repeated=False)
    assert torch.equal(old.test_probs[0], new.test_probs[0])
    with pytest.raises(Exception, match='allow_repeats'):
        old.update(idx, [0], probs=src, repeated=True)


def test_vote_scene_over_a_small_and_a_large_room_in_both_modes():
    """vote_scene with an S3DIS-form sampler, one room below num_points: runs eagerly and graphed.  Which points are voted for, and how
    often, is the sampler's business and must be identical in both modes; each mode gives the same bytes when repeated.  (The vote VALUES
    of the two modes differ by design: a graphed crop after the first draws its coarse subsets from the collate graph's counter, an eager
    one from torch.randperm -- vote_scene's docstring.)"""
    from crfconv_amd import models
    sizes, k, C, n_crops = (9000, 2000), 4096, 13, 5
    sc = rooms(sizes, 51)
    torch.manual_seed(3)
    net = models.PointConvBig(6, C, use_crf=True, steps=3).to(DEV).eval()
    tables = {}
    for graphed in (False, True):
        for rep in range(2):
            smp, _ = s3dis_pair(sc, k, generator=torch.Generator().manual_seed(77))
            votes = VoteAccumulator(sizes, C, smooth=0.95, device=DEV, track_visits=True, allow_repeats=True)
            seen = []
            vote_scene(smp, net, votes, n_crops, generator=torch.Generator().manual_seed(3), graphed=graphed,
                       on_crop=lambda data, logits, point_idx: seen.append(point_idx.reshape(-1).clone()))
            votes.check()
            assert len(seen) == n_crops and all(s.numel() == k for s in seen)
            assert any(s.unique().numel() == sizes[1] for s in seen)           # the small room was drawn, whole and padded
            for tp in votes.test_probs:
                assert bool(torch.isfinite(tp).all())
            tables[(graphed, rep)] = ([tp.clone() for tp in votes.test_probs], [v.clone() for v in votes.visits])
        for a, b in zip(tables[(graphed, 0)][0] + tables[(graphed, 0)][1], tables[(graphed, 1)][0] + tables[(graphed, 1)][1]):
            assert torch.equal(a, b), graphed
    for c in range(2):
        assert torch.equal(tables[(False, 0)][1][c], tables[(True, 0)][1][c])  # visit counts: the same crops, each point once per crop
        assert torch.equal(tables[(False, 0)][0][c].sum(1) > 0, tables[(True, 0)][0][c].sum(1) > 0)
    # without allow_repeats the S3DIS form is refused rather than raced
    smp, _ = s3dis_pair(sc, k)
    with pytest.raises(Exception, match='allow_repeats'):
        vote_scene(smp, net, VoteAccumulator(sizes, C, device=DEV), 1)
