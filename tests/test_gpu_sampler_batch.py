"""-m gpu: PossibilitySampler.get_batch (csrc/sampler.hip) -- B crops per call, every decision on the device -- against the fixture
captured from the reference (g9_eval.npz), against B consecutive get_random calls of a twin sampler (bit for bit), against the numpy
twin of its draws, inside a captured graph, and as the input stage of data.CollateGraph / CollatePipeline(sampler=)."""
import numpy as np
import pytest
import torch

import _seeded as S
from gpu_util import DEV, t
from crfconv_amd import transforms as T
from crfconv_amd.data import Data
from crfconv_amd.sampling import PossibilitySampler

pytestmark = pytest.mark.gpu


def train_chain(generator=None):
    return T.Compose([
        T.RandomRotate(degrees=180, axis=2),
        T.RandomScaleAnisotropic(scales=[0.8, 1.2], anisotropic=True),
        T.RandomSymmetry(axis=[True, False, False]),
        T.RandomNoise(sigma=0.001, clip=0.05),
        T.DropFeature(drop_proba=0.2, feature_name='rgb'),
        T.AddFeatsByKeys(list_add_to_x=[True, True], feat_names=['pos', 'rgb'], delete_feats=[False, True]),
    ], generator=generator or torch.Generator().manual_seed(99))


def scene(sizes, seed, box=(60.0, 60.0, 15.0)):
    """Clouds of the generator of test_possibility_sampler_full_size_properties, with colours, labels 0 .. 7 and start possibilities."""
    gen = torch.Generator().manual_seed(seed)
    pts = [(torch.rand(n, 3, generator=gen) * torch.tensor(box)).to(DEV) for n in sizes]
    rgb = [torch.rand(n, 3, generator=gen).to(DEV) for n in sizes]
    labels = [torch.randint(0, 8, (n,), generator=gen).to(DEV) for n in sizes]
    poss = [(torch.randn(n, dtype=torch.float64, generator=gen) * 1e-3) for n in sizes]
    return pts, rgb, labels, poss


CW = np.linspace(0.5, 2.0, 8)


def pair(sc, k, split='train', **kw):
    """Two samplers in the same state: the one under test and its twin."""
    pts, rgb, labels, poss = sc
    mk = lambda: PossibilitySampler(pts, rgb=rgb, labels=labels, num_points=k, class_weight=CW, split=split,      # noqa: E731
                                    possibility=[p.clone() for p in poss], **kw)
    return mk(), mk()


def assert_equals_twin_loop(batch, noise, perm, twin, B):
    """`batch` = what B consecutive get_random(noise_b, perm_b) calls on `twin` give, bit for bit."""
    for b in range(B):
        d = twin.get_random(noise=noise[b], perm=perm[b])
        assert int(batch.cloud_idx[b, 0]) == int(d.cloud_idx[0]), b
        assert torch.equal(batch.point_idx[b], d.point_idx), b
        assert torch.equal(batch.pos[b], d.pos), b
        assert torch.equal(batch.y[b], d.y), b
        assert torch.equal(batch.center[b], d.center), b
        assert torch.equal(batch.x[b, :, :3], d.pos), b
        assert torch.equal(batch.x[b, :, 3:], d.rgb), b


def assert_same_state(a, b):
    for c, (p, q) in enumerate(zip(a.possibility, b.possibility)):
        assert torch.equal(p, q), 'possibility table of cloud %d' % c
    assert torch.equal(a._minv, b._minv) and torch.equal(a._mini, b._mini)


@pytest.mark.parametrize('split', ['train', 'test'])
def test_batch_reproduces_the_reference_fixture(golden, split):
    """ONE get_batch(6) against six consecutive Semantic3D._get_random draws (fixture; they alternate clouds 0, 1, 1, 0, 0, 0): cloud
    ids, crop membership, centred coordinates, colours, labels and the final float64 possibility tables -- all bit-exact."""
    g = golden('g9_eval.npz')
    clouds = [t(g['s_cloud0']), t(g['s_cloud1'])]
    labels = [t(g['s_labels0'].astype(np.int64)), t(g['s_labels1'].astype(np.int64))]
    rgb = [t(g['s_rgb0']), t(g['s_rgb1'])]
    smp = PossibilitySampler(clouds, rgb=rgb, labels=labels, num_points=1500, class_weight=g['s_cw'][0],
                             label_to_idx={l: i for i, l in enumerate(range(1, 9))}, split=split,
                             possibility=[g['s_poss0'], g['s_poss1']])
    noise = np.stack([g['s_%s_%d_noise' % (split, i)] for i in range(6)])
    d = smp.get_batch(6, noise=noise, perm=False)
    assert d.pos.shape == (6, 1500, 3) and d.x.shape == (6, 1500, 6) and d.y.shape == (6, 1500)
    assert d.point_idx.shape == (6, 1500) and d.cloud_idx.shape == (6, 1) and d.center.shape == (6, 3)
    seen = []
    for draw in range(6):
        tag = 's_%s_%d_' % (split, draw)
        assert int(d.cloud_idx[draw, 0]) == int(g[tag + 'cloud'][0])
        seen.append(int(d.cloud_idx[draw, 0]))
        idx, ref_idx = d.point_idx[draw].cpu().numpy(), g[tag + 'point_idx'].astype(np.int64)
        o, ro = np.argsort(idx), np.argsort(ref_idx)
        assert np.array_equal(idx[o], ref_idx[ro])
        assert np.array_equal(d.pos[draw].cpu().numpy()[o], g[tag + 'pos'][ro])
        assert np.array_equal(d.x[draw, :, :3].cpu().numpy()[o], g[tag + 'pos'][ro])
        assert np.array_equal(d.x[draw, :, 3:].cpu().numpy()[o], g[tag + 'rgb'][ro].astype(np.float32))
        assert np.array_equal(d.y[draw].cpu().numpy()[o], g[tag + 'y'][ro])
    assert len(set(seen)) == 2                                # the device-side cloud choice is exercised
    assert np.array_equal(smp.min_possibility, g['s_%s_5_min_possibility' % split])
    for c in range(2):
        assert np.array_equal(smp.possibility[c].cpu().numpy(), g['s_%s_possibility%d' % (split, c)])


@pytest.mark.parametrize('k', [40960, 65536])
@pytest.mark.parametrize('sizes', [(1 << 20,), (300000, 150000, 70000)], ids=['one_cloud_1M', 'three_clouds'])
def test_batch_equals_the_twin_loop_at_size(sizes, k):
    B = 4
    smp, twin = pair(scene(sizes, 3), k, generator=torch.Generator().manual_seed(5))
    batch, noise, perm = smp.get_batch(B, return_draws=True)
    assert noise.shape == (B, 3) and perm.shape == (B, k)
    assert torch.equal(perm.sort(dim=1).values, torch.arange(k, device=DEV).repeat(B, 1))
    assert_equals_twin_loop(batch, noise, perm, twin, B)
    assert_same_state(smp, twin)
    for b in range(B):
        assert batch.point_idx[b].unique().numel() == k


def test_ties_go_to_the_lower_point_id():
    """2 000 distinct points, each in 8 scattered rows, k not a multiple of 8: the ball's boundary cuts through a run of equal keys."""
    gen = torch.Generator().manual_seed(11)
    base = torch.rand(2000, 3, generator=gen) * torch.tensor([10.0, 10.0, 3.0])
    rows = torch.arange(2000).repeat(8)[torch.randperm(16000, generator=gen)]
    pts = base[rows].to(DEV)
    sc = ([pts], [torch.rand(16000, 3, generator=gen).to(DEV)], [torch.randint(0, 8, (16000,), generator=gen).to(DEV)],
          [torch.randn(16000, dtype=torch.float64, generator=gen) * 1e-3])
    for k in (1001, 4003):
        smp, twin = pair(sc, k, generator=torch.Generator().manual_seed(6))
        batch, noise, perm = smp.get_batch(3, return_draws=True)
        assert_equals_twin_loop(batch, noise, perm, twin, 3)
        assert_same_state(smp, twin)
        # nearest first (identity shuffle): equal keys in ascending point order, also across the boundary
        smp, twin = pair(sc, k)
        batch, noise, perm = smp.get_batch(2, perm=False, return_draws=True)
        assert torch.equal(perm, torch.arange(k, device=DEV).repeat(2, 1))
        assert_equals_twin_loop(batch, noise, [False, False], twin, 2)
        assert_same_state(smp, twin)


@pytest.mark.parametrize('sizes,k', [((4097, 256, 8193), 256), ((4096, 257), 257)], ids=['tile_edges', 'one_row_in_the_second_block'])
def test_batch_equals_the_twin_loop_at_the_edge_shapes(sizes, k):
    """The shapes at which the pieces shared by the batch and the single-crop path (csrc/crop_common.hpp) can go wrong: a second select
    tile holding one point (4097), three tiles (8193), n == k (the select takes the whole cloud; 256: one distance block), and k = 257,
    where the second distance block holds one row -- the farthest -- so d_max must come from across the blocks.  One point of the
    n == k cloud starts lowest, so that cloud is certainly drawn first; the update lifts that point and the other clouds follow (the
    sequence was checked beforehand with a numpy restatement on the host: clouds 1, 2, 2, 0, 2 and 1, 0, 0, 0, 0)."""
    B = 5
    sc = scene(sizes, 61 if k == 256 else 62)
    whole = sizes.index(k)
    sc[3][whole][0] -= 1e-2
    smp, twin = pair(sc, k)
    batch, noise, perm = smp.get_batch(B, seed=1, return_draws=True)
    drawn = [int(c) for c in batch.cloud_idx[:, 0]]
    print('clouds drawn:', drawn)
    assert len(set(drawn)) >= 2 and whole in drawn
    assert torch.equal(perm.sort(dim=1).values, torch.arange(k, device=DEV).repeat(B, 1))
    assert_equals_twin_loop(batch, noise, perm, twin, B)
    assert_same_state(smp, twin)


def test_device_draws_are_the_host_twins():
    B, k = 5, 3000
    smp, _ = pair(scene((20000, 9000), 4), k, noise_scale=0.35)
    counter = torch.full((1,), 41, dtype=torch.int64, device=DEV)
    _, noise, perm = smp.get_batch(B, seed=777, counter=counter, return_draws=True)
    assert int(counter.item()) == 41                          # an explicit counter belongs to the caller
    host = PossibilitySampler.draws(777, 41, B, k=k, noise_scale=0.35)
    assert np.array_equal(perm.cpu().numpy(), host['perm'])
    err = np.abs(noise.cpu().numpy() - host['noise']).max()
    print('max |noise - host twin| = %.3e (bound %.3e)' % (err, 1e-12 * 0.35))
    assert err <= 1e-12 * 0.35
    # the sampler's own counter advances before the draw: the first call reads 1
    _, noise, perm = smp.get_batch(B, seed=778, return_draws=True)
    host = PossibilitySampler.draws(778, 1, B, k=k, noise_scale=0.35)
    assert np.array_equal(perm.cpu().numpy(), host['perm'])
    assert np.abs(noise.cpu().numpy() - host['noise']).max() <= 1e-12 * 0.35
    assert smp.state_dict()['counter'] == 1


def test_captured_batch_draws_new_crops_at_every_replay():
    """torch.cuda.graph around get_batch(out=): a host synchronisation inside would make the capture fail."""
    B, k = 3, 4096
    smp, twin = pair(scene((50000, 30000), 7), k)
    out = Data(pos=torch.empty((B, k, 3), device=DEV), x=torch.empty((B, k, 6), device=DEV),
               y=torch.empty((B, k), dtype=torch.int64, device=DEV), point_idx=torch.empty((B, k), dtype=torch.int64, device=DEV),
               cloud_idx=torch.empty((B, 1), dtype=torch.int64, device=DEV), center=torch.empty((B, 3), dtype=torch.float64, device=DEV))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        snap = smp.snapshot()
        smp.get_batch(B, out=out, seed=4242)                 # warm-up (tables, workspace)
        smp.restore(snap)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert_same_state(smp, twin)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = smp.get_batch(B, out=out, seed=4242)
    assert got.pos is out.pos and got.x is out.x and got.y is out.y and got.point_idx is out.point_idx
    assert_same_state(smp, twin)                              # a capture runs nothing
    seen = []
    for i in range(3):
        graph.replay()
        ref = twin.get_batch(B, seed=4242)
        for name in ('pos', 'x', 'y', 'point_idx', 'cloud_idx', 'center'):
            assert torch.equal(getattr(out, name), getattr(ref, name)), (i, name)
        assert_same_state(smp, twin)
        seen.append(out.point_idx.clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2]) and not torch.equal(seen[0], seen[2])
    assert smp.state_dict()['counter'] == 3


def static_batch(B, N, seed=500):
    import crfconv_amd
    pos = np.stack([S.make_cloud(seed + b, N, box=(2, 2, 1)) for b in range(B)])
    feats = np.concatenate([pos, S.uniform(seed, 'rgb', (B, N, 3), 0, 1)], -1)
    return crfconv_amd.multiscale_compute(t(pos), x=t(feats), y=t(S.integers(seed, 'y', (B, N), 0, 14)),
                                          point_idx=torch.zeros((B, N), dtype=torch.int64, device=DEV),
                                          cloud_idx=torch.zeros((B, 1), dtype=torch.int64, device=DEV),
                                          generator=torch.Generator().manual_seed(1))


def same_batch(a, b):
    for name in ('x', 'y', 'point_idx', 'cloud_idx'):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    for la, lb in zip(a.multiscale, b.multiscale):
        for name in ('pos', 'neighbor_idx', 'sub_idx', 'up_idx'):
            u, v = getattr(la, name), getattr(lb, name)
            assert (u is None and v is None) or torch.equal(u, v), name


def small_scene(seed=21):
    return scene((20000, 12000), seed, box=(20.0, 20.0, 5.0))


def test_collate_graph_draws_its_own_input():
    import crfconv_amd
    from crfconv_amd.data import CollateGraph
    B, N = 2, 4096
    chain = train_chain()
    smp, twin = pair(small_scene(), N)
    static = static_batch(B, N)
    cg = CollateGraph(static, generator=torch.Generator().manual_seed(9), augment=chain, sampler=smp)
    for i in range(3):
        assert cg.run() is static
        counter = torch.full((1,), i + 1, dtype=torch.int64, device=DEV)
        assert torch.equal(cg.counter, counter)
        d = twin.get_batch(B, seed=cg.seed, counter=counter)
        assert_same_state(smp, twin)                          # (i = 0: the warm-up pass before the capture consumed no crop)
        chain.apply_batch(d.pos, d.x, cg.seed, counter)
        order = crfconv_amd.data.morton_order(d.pos)
        assert torch.equal(order, cg.order)
        ref = crfconv_amd.multiscale_compute(d.pos, x=d.x, y=d.y, point_idx=d.point_idx, cloud_idx=d.cloud_idx,
                                             choices=[c.clone() for c in cg.choices], sort='morton', order=order)
        same_batch(static, ref)
        assert torch.equal(static.x[..., :3], static.multiscale[0].pos)
    # resume: sampler + graph state into fresh objects
    smp2 = PossibilitySampler(smp.points, rgb=smp.rgb, labels=small_scene()[2], num_points=N, class_weight=CW)      # another start state
    smp2.load_state_dict(smp.state_dict())
    assert_same_state(smp2, smp)
    static2 = static_batch(B, N, 510)
    cg2 = CollateGraph(static2, generator=torch.Generator().manual_seed(10), augment=train_chain(torch.Generator().manual_seed(3)),
                       sampler=smp2)
    cg2.load_state_dict(cg.state_dict())
    cg.run()
    cg2.run()
    same_batch(static2, static)
    assert_same_state(smp2, smp)
    assert cg2.state_dict()['counter'] == 4


def test_pipeline_slots_draw_in_submission_order():
    from crfconv_amd.data import CollatePipeline
    B, N = 2, 4096
    smp, twin = pair(small_scene(23), N)
    statics = [static_batch(B, N, 600 + s) for s in range(2)]
    pipe = CollatePipeline(statics, generator=torch.Generator().manual_seed(3), augment=train_chain(), sampler=smp)
    for rnd in range(2):
        for s in range(2):
            pipe.submit(s)
        for s in range(2):
            batch = pipe.acquire(s)
            torch.cuda.current_stream().synchronize()
            counter = torch.full((1,), rnd + 1, dtype=torch.int64, device=DEV)
            d = twin.get_batch(B, seed=pipe.graphs[s].seed, counter=counter)
            assert torch.equal(batch.cloud_idx, d.cloud_idx), (rnd, s)
            assert torch.equal(batch.point_idx.sort(dim=1).values, d.point_idx.sort(dim=1).values), (rnd, s)
            assert torch.equal(batch.x[..., :3], batch.multiscale[0].pos)
            pipe.release(s)
    torch.cuda.synchronize()
    assert_same_state(smp, twin)
    assert [g.state_dict()['counter'] for g in pipe.graphs] == [2, 2]


def test_captured_step_trains_on_sampler_drawn_batches():
    """Plumbing only: one train.CapturedStep over the collate graph's target, three steps on crops the sampler drew."""
    import torch.nn.functional as F
    from crfconv_amd import models
    from crfconv_amd.data import CollateGraph
    from crfconv_amd.train import CapturedStep
    B, N = 2, 4096
    smp, _ = pair(small_scene(25), N)
    static = static_batch(B, N)
    cg = CollateGraph(static, generator=torch.Generator().manual_seed(12), augment=train_chain(), sampler=smp)
    cg.run()
    shapes = {name: tuple(getattr(static, name).shape) for name in ('x', 'y', 'point_idx', 'cloud_idx')}
    torch.manual_seed(6)
    net = models.PointConvBig(6, 13, True, 3).to(DEV).train()
    opt = torch.optim.SGD(net.parameters(), lr=1e-2, momentum=0.95)
    step = CapturedStep(net, opt, lambda out, d: F.cross_entropy(out, d.y.reshape(-1) - 1, ignore_index=-1), static)
    drawn = []
    for i in range(3):
        cg.run()
        loss = step()
        assert torch.isfinite(loss).item()
        drawn.append(static.point_idx.clone())
    assert not torch.equal(drawn[0], drawn[1]) and not torch.equal(drawn[1], drawn[2])
    assert shapes == {name: tuple(getattr(static, name).shape) for name in shapes}
    assert cg.state_dict()['counter'] == 4


def test_errors():
    from crfconv_amd.data import CollateGraph
    pts, rgb, labels, poss = scene((5000, 900), 2)
    smp = PossibilitySampler(pts, rgb=rgb, labels=labels, num_points=1000, class_weight=CW, possibility=poss)
    with pytest.raises(ValueError, match='cloud 1'):
        smp.get_batch(2)
    ok = PossibilitySampler(pts[:1], rgb=rgb[:1], labels=labels[:1], num_points=4096, class_weight=CW, possibility=poss[:1])
    static = static_batch(2, 4096)
    with pytest.raises(ValueError, match='device_draw'):
        CollateGraph(static, sampler=ok, device_draw=False)
    with pytest.raises(ValueError, match='take none'):
        CollateGraph(static, sampler=ok).run(static.multiscale[0].pos)
    with pytest.raises(ValueError):
        ok.get_batch(2, noise=np.zeros((3, 3)))
