"""-m gpu: votes keyed by device cloud ids (VoteAccumulator.update_batch / confusion / scores, csrc/evaluate.hip) and the batched,
replayed inference loop built on them (sampling.SceneVoter) -- against numpy's sequential update, today's per-sample entries, the
np.add.at restatement of the confusion matrix, and twin samplers in the same state."""
import numpy as np
import pytest
import torch

from gpu_util import DEV, t
from crfconv_amd.sampling import PossibilitySampler, SceneVoter, VoteAccumulator
from s3dis_restatement import vote_repeated
from test_host_scene_voter import confusion_restated, scores_restated

pytestmark = pytest.mark.gpu


def softmax_rows(rng, shape):
    z = rng.standard_normal(shape).astype(np.float32)
    e = np.exp(z - z.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(np.float32)


def overlapping_batch(rng):
    """B = 4 samples of N = 128 rows over clouds of 300 / 700 / 50 points: samples 0, 1 and 3 name cloud 1, samples 0 and 1 share 64 points."""
    idx = np.stack([np.arange(128), np.arange(64, 192), rng.choice(300, 128, replace=False), rng.choice(700, 128, replace=False)]).astype(np.int64)
    cloud = np.array([[1], [1], [0], [1]], np.int64)
    assert np.intersect1d(idx[0], idx[1]).size == 64
    assert np.intersect1d(idx[3], np.arange(192)).size > 0          # (sample 3 meets both of them again)
    for row in idx:
        assert np.unique(row).size == 128
    return idx, cloud


def test_batch_update_equals_the_per_sample_loop_and_numpy_with_overlapping_samples():
    sizes, C, N, B, smooth = (300, 700, 50), 5, 128, 4, 0.98
    rng = np.random.default_rng(21)
    idx, cloud = overlapping_batch(rng)
    new = VoteAccumulator(sizes, C, smooth=smooth, device=DEV, track_visits=True)
    old = VoteAccumulator(sizes, C, smooth=smooth, device=DEV, track_visits=True)
    ref = [np.zeros((n, C), np.float32) for n in sizes]
    ref_visits = [np.zeros(n, np.int32) for n in sizes]
    cloud_dev = t(cloud)
    assert cloud_dev.shape == (B, 1)
    for call in range(3):                                            # the later calls meet non-zero old rows
        p = softmax_rows(rng, (B, N, C))
        new.update_batch(t(idx), cloud_dev, probs=t(p))
        old.update(t(idx), [int(c) for c in cloud[:, 0]], probs=t(p).reshape(B * N, C))
        for b in range(B):                                           # trainval.py:184-189
            c = int(cloud[b, 0])
            ref[c][idx[b]] = smooth * ref[c][idx[b]] + (1 - smooth) * p[b]
            ref_visits[c][idx[b]] += 1
        assert ref[1].dtype == np.float32
    new.check()
    for c in range(3):
        assert np.array_equal(new.test_probs[c].cpu().numpy(), ref[c]), c
        assert np.array_equal(new.visits[c].cpu().numpy(), ref_visits[c]), c
        assert torch.equal(new.test_probs[c], old.test_probs[c]) and torch.equal(new.visits[c], old.visits[c]), c
    assert int(ref_visits[1][64:128].min()) >= 6                     # the shared points were updated twice per call, in batch order
    assert not bool(new.test_probs[2].any()) and not bool(new.visits[2].any())      # cloud 2 (50 points, below N) is never named

    # logits: against today's kernel only (its soft-max is the device's expf); cloud ids as a [B] tensor, no visit tables
    new, old = VoteAccumulator(sizes, C, smooth=smooth, device=DEV), VoteAccumulator(sizes, C, smooth=smooth, device=DEV)
    for call in range(3):
        z = t(rng.standard_normal((B * N, C)).astype(np.float32) * 3)
        new.update_batch(t(idx), cloud_dev[:, 0], logits=z)
        old.update(t(idx), cloud_dev, logits=z)
    new.check()
    for c in range(3):
        assert torch.equal(new.test_probs[c], old.test_probs[c]), c
    assert bool(new.test_probs[1].any()) and not bool(new.test_probs[2].any())
    # the tables are the accumulator's own: a replaced one is refused, not silently missed
    new.test_probs[0] = torch.zeros_like(new.test_probs[0])
    with pytest.raises(Exception, match='replaced'):
        new.update_batch(t(idx), cloud_dev, logits=z)


def test_repeated_form_equals_numpys_fancy_assignment():
    """Sample 0: the padded crop of a 50-point cloud in 128 rows (the sampler's own padding pattern composed with a shuffle); sample 1:
    distinct rows of another cloud; sample 2: the small cloud again, padded differently -- in ONE call."""
    sizes, C, N, smooth = (50, 400), 6, 128, 0.95
    runs = []
    for run in range(2):
        rng = np.random.default_rng(8)
        votes = VoteAccumulator(sizes, C, smooth=smooth, device=DEV, track_visits=True, allow_repeats=True)
        ref = [np.zeros((n, C), np.float32) for n in sizes]
        ref_visits = [np.zeros(n, np.int32) for n in sizes]
        cloud = np.array([0, 1, 0], np.int64)
        for call in range(2):
            choice = PossibilitySampler.draws(123, call, 2, k=N, kc=[50, 50])['choice']
            idx = np.stack([rng.permutation(50)[choice[0]], rng.choice(400, N, replace=False), rng.permutation(50)[choice[1]]]).astype(np.int64)
            assert np.unique(idx[0]).size == 50 and np.unique(idx[2]).size == 50 and np.unique(idx[1]).size == N
            p = softmax_rows(rng, (3, N, C))
            votes.update_batch(t(idx), t(cloud), probs=t(p))
            for b in range(3):
                vote_repeated(ref[cloud[b]], ref_visits[cloud[b]], idx[b], p[b], smooth)
        votes.check()
        for c in range(2):
            assert np.array_equal(votes.test_probs[c].cpu().numpy(), ref[c]), c
            assert np.array_equal(votes.visits[c].cpu().numpy(), ref_visits[c]), c
            assert bool((votes._last[c] == -1).all()), c
        assert int(votes.visits[0].min()) == int(votes.visits[0].max()) == 4
        runs.append([tp.clone() for tp in votes.test_probs])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    with pytest.raises(Exception, match='allow_repeats'):
        VoteAccumulator(sizes, C, device=DEV).update_batch(t(idx), t(cloud), probs=t(p), repeated=True)


@pytest.mark.parametrize('repeated', [False, True])
def test_bad_rows_and_bad_cloud_ids_are_counted_and_skipped(repeated):
    """One row index = n, one = -1, one sample whose cloud id is n_clouds: range checks in the kernels, nothing is addressed out of range;
    check() reports 2 + N and every other row was applied."""
    sizes, C, N, smooth = (300, 700), 5, 128, 0.98
    rng = np.random.default_rng(5)
    idx = np.stack([rng.choice(300, N, replace=False), rng.choice(300, N, replace=False), rng.choice(700, N, replace=False)]).astype(np.int64)
    idx[0, 5], idx[0, 9] = 300, -1
    cloud = np.array([[0], [2], [1]], np.int64)
    p = softmax_rows(rng, (3, N, C))
    votes = VoteAccumulator(sizes, C, smooth=smooth, device=DEV, track_visits=True, allow_repeats=repeated)
    votes.update_batch(t(idx), t(cloud), probs=t(p))
    with pytest.raises(IndexError, match=r'^%d point' % (N + 2)):
        votes.check()
    ref = [np.zeros((n, C), np.float32) for n in sizes]
    ref_visits = [np.zeros(n, np.int32) for n in sizes]
    good = np.ones(N, bool)
    good[[5, 9]] = False
    vote_repeated(ref[0], ref_visits[0], idx[0][good], p[0][good], smooth)
    vote_repeated(ref[1], ref_visits[1], idx[2], p[2], smooth)
    for c in range(2):
        assert np.array_equal(votes.test_probs[c].cpu().numpy(), ref[c]), c
        assert np.array_equal(votes.visits[c].cpu().numpy(), ref_visits[c]), c
        if repeated:
            assert bool((votes._last[c] == -1).all()), c
    assert int(votes.visits[0].sum()) == N - 2 and int(votes.visits[1].sum()) == N


def test_update_batch_is_capturable_and_replays_follow_the_tensors():
    sizes, C, N, B, smooth = (300, 700, 50), 5, 128, 4, 0.98
    rng = np.random.default_rng(33)
    idx, cloud = overlapping_batch(rng)
    graphed = VoteAccumulator(sizes, C, smooth=smooth, device=DEV, track_visits=True)
    eager = VoteAccumulator(sizes, C, smooth=smooth, device=DEV, track_visits=True)
    s_idx, s_cloud, s_probs = t(idx), t(cloud), t(softmax_rows(rng, (B, N, C)))
    graphed.update_batch(s_idx, s_cloud, probs=s_probs)               # eagerly once: the descriptor table is built outside the capture
    eager.update_batch(s_idx.clone(), s_cloud.clone(), probs=s_probs.clone())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        graphed.update_batch(s_idx, s_cloud, probs=s_probs)
    for rep in range(3):
        # new contents in place: other points, other clouds (cloud 0 holds 300 points: rows stay below 300), other votes
        new_idx = np.stack([rng.choice(300, N, replace=False) for _ in range(B)]).astype(np.int64)
        new_cloud = rng.integers(0, 2, (B, 1)).astype(np.int64)
        s_idx.copy_(t(new_idx))
        s_cloud.copy_(t(new_cloud))
        s_probs.copy_(t(softmax_rows(rng, (B, N, C))))
        graph.replay()
        eager.update_batch(s_idx.clone(), s_cloud.clone(), probs=s_probs.clone())
    graphed.check()
    for c in range(3):
        assert torch.equal(graphed.test_probs[c], eager.test_probs[c]), c
        assert torch.equal(graphed.visits[c], eager.visits[c]), c
    assert int(graphed.visits[0].sum()) + int(graphed.visits[1].sum()) == 4 * B * N and not bool(graphed.visits[2].any())


def vote_table(rng, n, C):
    """Rows of random votes, among them all-zero rows (unvoted points) and rows whose maximum is held by two or three classes."""
    tb = rng.random((n, C)).astype(np.float32)
    tb[rng.choice(n, n // 7, replace=False)] = 0
    tied = rng.choice(n, n // 5, replace=False)
    tb[tied, rng.integers(0, C, tied.size)] = 2.0
    tb[tied, rng.integers(0, C, tied.size)] = 2.0
    tb[tied[::3], rng.integers(0, C, tied[::3].size)] = 2.0
    return tb


def test_confusion_and_scores_against_numpy():
    C = 5
    rng = np.random.default_rng(17)
    sizes = (700, 300)
    tables = [vote_table(rng, n, C) for n in sizes]
    assert int((tables[0].sum(1) == 0).sum()) >= 50 and int(((tables[0] == 2.0).sum(1) >= 2).sum()) >= 50
    votes = VoteAccumulator(sizes, C, device=DEV)
    for tp, tb in zip(votes.test_probs, tables):
        tp.copy_(t(tb))
    labels = [rng.integers(-1, C + 1, n) for n in sizes]              # -1: the ignore value below; C: out of range above
    assert all((lab == -1).any() and (lab == C).any() for lab in labels)
    # direct form
    hist = votes.confusion(0, t(labels[0]))
    want = confusion_restated(tables[0], labels[0])
    assert hist.dtype == torch.int64 and hist.shape == (C, C)
    assert np.array_equal(hist.cpu().numpy(), want)
    assert int(want.sum()) == int(((labels[0] >= 0) & (labels[0] < C)).sum()) and want[:, 0].sum() > want[:, 1].sum()   # zero rows -> class 0
    # proj_idx form: 3000 rows naming the 700 points, raw labels 0 .. C + 1 with label_shift = 1, one projection index out of range
    proj = rng.integers(0, 700, 3000)
    full = rng.integers(-1, C + 1, 3000) + 1
    proj_bad = proj.copy()
    proj_bad[77] = 700
    keep = np.arange(3000) != 77
    out = votes.confusion(0, t(full), proj_idx=t(proj_bad), label_shift=1)
    want_proj = confusion_restated(tables[0], full[keep], proj[keep], label_shift=1)
    assert np.array_equal(out.cpu().numpy(), want_proj)
    with pytest.raises(IndexError, match=r'^1 point'):
        votes.check()
    votes._bad.zero_()
    # accumulation over two calls into one matrix
    again = votes.confusion(0, t(full), proj_idx=t(proj), label_shift=1, out=out)
    assert again is out
    assert np.array_equal(out.cpu().numpy(), want_proj + confusion_restated(tables[0], full, proj, label_shift=1))
    # scores = the host restatement, both clouds, with and without class proportions, direct and projected
    projs = [proj, rng.integers(0, 300, 1000)]
    fulls = [full - 1, rng.integers(-1, C + 1, 1000)]
    prop = np.array([np.sum([np.sum(lab == c) for lab in fulls]) for c in range(C)], np.float32)        # trainval.py:222-224
    for kw in ({}, {'class_proportions': prop}):
        miou, ious = votes.scores([t(lab) for lab in labels], **kw)
        ref_miou, ref_ious = scores_restated(tables, labels, **kw)
        assert np.array_equal(ious, ref_ious) and miou == ref_miou and ious.shape == (C,)
        miou, ious = votes.scores([t(lab) for lab in fulls], proj=[t(p) for p in projs], **kw)
        ref_miou, ref_ious = scores_restated(tables, fulls, proj=projs, **kw)
        assert np.array_equal(ious, ref_ious) and miou == ref_miou
        assert 0.0 < miou < 1.0
    votes.check()


# ------------------------------------------------------------------------------------------------------------- SceneVoter end to end
def rooms(sizes, seed, box=(6.0, 5.0, 3.0)):
    gen = torch.Generator().manual_seed(seed)
    pts = [(torch.rand(n, 3, generator=gen) * torch.tensor(box)).to(DEV) for n in sizes]
    rgb = [torch.rand(n, 3, generator=gen).to(DEV) for n in sizes]
    labels = [torch.randint(0, 13, (n,), generator=gen).to(DEV) for n in sizes]
    poss = [(torch.randn(n, dtype=torch.float64, generator=gen) * 1e-3) for n in sizes]
    return pts, rgb, labels, poss


def make_sampler(sc, k, form):
    pts, rgb, labels, poss = sc
    kw = {'form': 's3dis', 'labels': labels} if form == 's3dis' else {'split': 'test'}
    return PossibilitySampler(pts, rgb=rgb, num_points=k, possibility=[p.clone() for p in poss], generator=torch.Generator().manual_seed(77), **kw)


def scene_voter_run(net, sc, sizes, k, B, steps, form):
    """One SceneVoter run with, per batch, (a) the eager forward of a clone of the static batch against the logits handed out and (b) the
    crops against a twin sampler in the same state; returns (vote tables, visits, recorded (point_idx, cloud_idx, logits))."""
    from crfconv_amd.data import morton_order
    C = 13
    smp, twin = make_sampler(sc, k, form), make_sampler(sc, k, form)
    s3dis = form == 's3dis'
    votes = VoteAccumulator(sizes, C, smooth=0.95 if s3dis else 0.98, device=DEV, track_visits=True, allow_repeats=s3dis)
    voter = SceneVoter(smp, net, votes, B, generator=torch.Generator().manual_seed(3))
    rec = []

    def on_batch(data, logits):
        i = len(rec)
        assert net.training is False
        assert logits.shape == (B * k, C) and data.point_idx.shape == (B, k) and data.cloud_idx.shape == (B, 1)
        # (b) step 0 is the sampler's own get_batch(B); replay i draws on the collate graph's seed and its counter = i
        d = twin.get_batch(B) if i == 0 else twin.get_batch(B, seed=voter.cg.seed, counter=torch.full((1,), i, dtype=torch.int64, device=DEV))
        order = morton_order(d.pos)
        assert torch.equal(data.point_idx, d.point_idx.gather(1, order)), i
        assert torch.equal(data.cloud_idx, d.cloud_idx), i
        assert torch.equal(data.order, order), i
        for p, q in zip(smp.possibility, twin.possibility):
            assert torch.equal(p, q), i
        # (a)
        with torch.no_grad():
            eager = net(data._apply(lambda v: v.clone()))
        assert torch.equal(eager, logits), i
        rec.append((data.point_idx.clone(), data.cloud_idx.clone(), logits.clone()))
    assert voter.run(n_batches=steps, on_batch=on_batch) is votes
    votes.check()
    assert len(rec) == steps == voter.batches and voter.graph is not None
    # the votes = today's per-sample update fed the recorded crops
    ref = VoteAccumulator(sizes, C, smooth=votes.smooth, device=DEV, track_visits=True, allow_repeats=s3dis)
    for point_idx, cloud_idx, logits in rec:
        ref.update(point_idx, cloud_idx, logits=logits)
    ref.check()
    for c in range(len(sizes)):
        assert torch.equal(votes.test_probs[c], ref.test_probs[c]), c
        assert torch.equal(votes.visits[c], ref.visits[c]), c
        assert bool(torch.isfinite(votes.test_probs[c]).all())
    return [tp.clone() for tp in votes.test_probs], [v.clone() for v in votes.visits], rec


@pytest.fixture(scope='module')
def net13():
    from crfconv_amd import models
    torch.manual_seed(3)
    return models.PointConvBig(6, 13, True, 3).to(DEV).eval()


def test_scene_voter_end_to_end_over_a_small_and_a_large_room(net13):
    sizes, k, B, steps = (9000, 2000), 4096, 2, 4                      # one eager step, three replayed
    sc = rooms(sizes, 51)
    sc[3][1] -= 4e-3                                                   # the small room holds the lowest possibility: the first crop is its
    first = scene_voter_run(net13, sc, sizes, k, B, steps, 's3dis')
    drawn = torch.cat([cloud.reshape(-1) for _, cloud, _ in first[2]]).tolist()
    print('rooms drawn:', drawn)
    assert 1 in drawn and 0 in drawn
    for point_idx, cloud, _ in first[2]:
        for b in range(B):
            if int(cloud[b, 0]) == 1:
                assert point_idx[b].unique().numel() == sizes[1]           # taken whole and padded to k rows
    assert net13.training is False
    # the same seeds again, the network left in training mode by the caller: identical bytes, and the mode is restored
    net13.train()
    try:
        second = scene_voter_run(net13, sc, sizes, k, B, steps, 's3dis')
        assert net13.training is True
    finally:
        net13.eval()
    for a, b in zip(first[0] + first[1], second[0] + second[1]):
        assert torch.equal(a, b)
    for (pa, ca, la), (pb, cb, lb) in zip(first[2], second[2]):
        assert torch.equal(pa, pb) and torch.equal(ca, cb) and torch.equal(la, lb)
    # an S3DIS-form sampler without allow_repeats is refused rather than raced
    with pytest.raises(Exception, match='allow_repeats'):
        SceneVoter(make_sampler(sc, k, 's3dis'), net13, VoteAccumulator(sizes, 13, device=DEV), B)


def test_scene_voter_over_a_semantic3d_form_sampler(net13):
    sizes, k, B, steps = (6000, 6000), 4096, 2, 2
    sc = rooms(sizes, 52, box=(20.0, 20.0, 5.0))
    tables, visits, rec = scene_voter_run(net13, sc, sizes, k, B, steps, 'semantic3d')
    assert all(p[b].unique().numel() == k for p, _, _ in rec for b in range(B))        # kNN crops: distinct rows
    assert sum(int(v.sum()) for v in visits) == steps * B * k
