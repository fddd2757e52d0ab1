"""-m gpu: crfconv_amd.transforms on the device (csrc/augment.hip) against a numpy restatement of the augmentation table of
trainval.py:26-36 (torch_geometric / torch_points3d semantics, restated below: parity with the real libraries is unpinned), and its
use inside the collate graph (data.CollateGraph / CollatePipeline(augment=)) and a training step."""
import numpy as np
import pytest
import torch

import _seeded as S
from gpu_util import DEV, t
from crfconv_amd import transforms as T

pytestmark = pytest.mark.gpu


def train_chain(generator=None, sigma=0.001, clip=0.05, axis=2, sym=(True, False, False)):
    return T.Compose([
        T.RandomRotate(degrees=180, axis=axis),
        T.RandomScaleAnisotropic(scales=[0.8, 1.2], anisotropic=True),
        T.RandomSymmetry(axis=list(sym)),
        T.RandomNoise(sigma=sigma, clip=clip),
        T.DropFeature(drop_proba=0.2, feature_name='rgb'),
        T.AddFeatsByKeys(list_add_to_x=[True, True], feat_names=['pos', 'rgb'], delete_feats=[False, True]),
    ], generator=generator or torch.Generator().manual_seed(99))


def restate(pos, rgb, params, noise, axis=2, flip_axes=1, clip=0.05, rotate=True, scale=True, use_noise=True, drop=True):
    """The table of the issue in float32 numpy, one singly rounded operation at a time, per crop:
    rotate pos <- pos @ M (x_a' = c x_a - s x_b, x_b' = s x_a + c x_b, (a, b) = (axis + 1, axis + 2) mod 3), scale pos *= s,
    flip pos_i <- max(pos_i) - pos_i, noise pos += clamp(noise, -clip, clip), drop rgb <- 0, x = [pos, rgb].
    Returns (pos, x, c_max of the lowest flipped axis or 0 per crop)."""
    pos = pos.astype(np.float32).copy()
    B = pos.shape[0]
    cm_first = np.zeros(B, np.float32)
    out_rgb = rgb.astype(np.float32).copy()
    for b in range(B):
        p = pos[b]
        c, s = np.float32(params[b, 0]), np.float32(params[b, 1])
        if rotate:
            ia, ib = (axis + 1) % 3, (axis + 2) % 3
            xa, xb = p[:, ia].copy(), p[:, ib].copy()
            p[:, ia] = c * xa - s * xb
            p[:, ib] = s * xa + c * xb
        if scale:
            p *= params[b, 2:5].astype(np.float32)
        flip = int(params[b, 5]) & flip_axes
        first = True
        for i in range(3):
            if (flip >> i) & 1:
                cm = p[:, i].max()
                if first:
                    cm_first[b], first = cm, False
                p[:, i] = cm - p[:, i]
        if use_noise:
            p += np.clip(noise[b], np.float32(-clip), np.float32(clip))
        if drop and params[b, 6] == 0:
            out_rgb[b] = 0
    return pos, np.concatenate([pos, out_rgb], -1), cm_first


def random_params(seed, B):
    r = np.random.default_rng(seed)
    th = r.uniform(-np.pi, np.pi, B)
    p = np.zeros((B, 8), np.float32)
    p[:, 0], p[:, 1] = np.cos(th), np.sin(th)
    p[:, 2:5] = r.uniform(0.8, 1.2, (B, 3))
    p[:, 5] = r.integers(0, 8, B)
    p[:, 6] = np.arange(B) % 2 if B > 1 else 0
    return p


@pytest.mark.parametrize('B', [1, 4])
@pytest.mark.parametrize('N', [1, 63, 64, 65, 1000, 40960, 65536])
def test_given_parameters_and_noise_match_the_restatement(B, N):
    axis = N % 3                                         # every rotation axis is seen
    chain = T.Compose([T.RandomRotate(180, axis=axis), T.RandomScaleAnisotropic([0.8, 1.2]), T.RandomSymmetry([True, True, True]),
                       T.RandomNoise(sigma=0.03, clip=0.05), T.DropFeature(0.2),
                       T.AddFeatsByKeys([True, True], ['pos', 'rgb'], delete_feats=[False, True])],
                      generator=torch.Generator().manual_seed(N))
    pos = S.uniform(N, 'pos', (B, N, 3), -20, 30)
    rgb = S.uniform(N, 'rgb', (B, N, 3), 0, 1)
    noise = S.uniform(N, 'noise', (B, N, 3), -0.1, 0.1)   # half of it beyond clip
    params = random_params(N, B)
    want_pos, want_x, want_cm = restate(pos, rgb, params, noise, axis=axis, flip_axes=7)
    dpos, dx = t(pos), t(np.concatenate([pos * 0 + 7, rgb], -1))     # (x[..., 0:3] is written from pos, whatever it held)
    counter = torch.zeros(1, dtype=torch.int64, device=DEV)
    pout = torch.full((B, 8), -1.0, device=DEV)
    chain.apply_batch(dpos, dx, 17, counter, params_out=pout, params_in=t(params), noise_in=t(noise))
    bound = 1e-6 * max(1.0, float(np.abs(want_pos).max()))
    np.testing.assert_allclose(dpos.cpu().numpy(), want_pos, rtol=0, atol=bound)
    np.testing.assert_allclose(dx.cpu().numpy(), want_x, rtol=0, atol=bound)
    assert torch.equal(dx[..., :3], dpos)
    po = pout.cpu().numpy()
    np.testing.assert_array_equal(po[:, :7], params[:, :7])
    np.testing.assert_array_equal(po[:, 7], want_cm)
    # noise beyond clip is clamped: without rotation / scale / flips / drop, pos moves by exactly clamp(noise)
    only = T.Compose([T.RandomNoise(sigma=0.03, clip=0.05)], generator=torch.Generator().manual_seed(1))
    dpos = t(pos)
    only.apply_batch(dpos, None, 17, counter, noise_in=t(noise))
    np.testing.assert_array_equal(dpos.cpu().numpy(), pos + np.clip(noise, np.float32(-0.05), np.float32(0.05)))
    # flips on, noise off: a flipped axis' minimum is EXACTLY 0 (max pass and apply pass compute rot.scale identically)
    flips = T.Compose([T.RandomRotate(180, axis=axis), T.RandomScaleAnisotropic([0.8, 1.2]), T.RandomSymmetry([True, True, True]),
                       T.AddFeatsByKeys([True], ['pos'])], generator=torch.Generator().manual_seed(2))
    params[:, 5] = 7
    dpos, dx3 = t(pos), t(np.zeros((B, N, 3), np.float32))
    flips.apply_batch(dpos, dx3, 17, counter, params_out=pout, params_in=t(params))
    got = dpos.cpu().numpy()
    np.testing.assert_array_equal(got.min(axis=1), 0.0)
    want_pos, _, want_cm = restate(pos, rgb, params, None, axis=axis, flip_axes=7, use_noise=False, drop=False)
    np.testing.assert_allclose(got, want_pos, rtol=0, atol=1e-6 * max(1.0, float(np.abs(want_pos).max())))
    np.testing.assert_array_equal(pout[:, 7].cpu().numpy(), want_cm)
    assert torch.equal(dx3, dpos)
    # keep bit 0: rgb exactly 0, x[..., 0:3] == pos bit for bit
    drop = T.Compose([T.RandomRotate(180, axis=axis), T.DropFeature(0.5), T.AddFeatsByKeys([True, True], ['pos', 'rgb'])],
                     generator=torch.Generator().manual_seed(3))
    params[:, 6] = 0
    dpos, dx = t(pos), t(np.concatenate([pos, rgb], -1))
    drop.apply_batch(dpos, dx, 17, counter, params_in=t(params))
    assert torch.equal(dx[..., 3:], torch.zeros_like(dx[..., 3:]))
    assert torch.equal(dx[..., :3], dpos)


def test_device_draws_are_the_host_twins():
    B, N = 256, 64
    chain = train_chain(sym=(True, True, False))
    counter = torch.full((1,), 41, dtype=torch.int64, device=DEV)
    pout = torch.empty((B, 8), device=DEV)
    pos = S.uniform(5, 'pos', (B, N, 3), -3, 3)
    chain.apply_batch(t(pos), t(np.zeros((B, N, 6), np.float32)), chain.seed, counter, params_out=pout)
    got = pout.cpu().numpy()
    host = chain.draws(chain.seed, 41, B)
    np.testing.assert_array_equal(got[:, 5], host['flip'])
    np.testing.assert_array_equal(got[:, 6], host['keep'])
    np.testing.assert_allclose(got[:, 2:5], host['scale'], rtol=0, atol=1e-6)
    np.testing.assert_allclose(got[:, 0], host['cos'], rtol=0, atol=1e-6)
    np.testing.assert_allclose(got[:, 1], host['sin'], rtol=0, atol=1e-6)
    assert 0 < host['flip'].astype(bool).sum() < B and 0 < (~host['keep']).sum() < B
    # the per-point noise: N(0, sigma) before the clamp (one cloud of 65 536 points x 3 axes)
    noise = T.Compose([T.RandomNoise(sigma=1.0, clip=100.0)], generator=torch.Generator().manual_seed(4))
    z = torch.zeros((1, 65536, 3), device=DEV)
    noise.apply_batch(z, None, 3, counter)
    v = z.double().cpu().numpy().ravel()
    n = v.size
    assert abs(v.mean()) < 4 / np.sqrt(n) and abs(v.var() - 1) < 4 * np.sqrt(2 / n), (v.mean(), v.var())
    assert abs((np.abs(v) < 1).mean() - 0.682689) < 4 * np.sqrt(0.22 / n)
    z2 = torch.zeros((1, 65536, 3), device=DEV)
    noise.apply_batch(z2, None, 3, counter)
    assert torch.equal(z, z2)                            # a function of (seed, counter): deterministic


def clouds(seed, B, N):
    pos = np.stack([S.make_cloud(seed + b, N, box=(2, 2, 1)) for b in range(B)])
    feats = np.concatenate([pos, S.uniform(seed, 'rgb', (B, N, 3), 0, 1)], -1)
    return t(pos), t(feats), t(S.integers(seed, 'y', (B, N), 0, 14))


def static_batch(B, N, seed=500):
    import crfconv_amd
    pos0, x0, y0 = clouds(seed, B, N)
    return crfconv_amd.multiscale_compute(pos0, x=x0, y=y0, generator=torch.Generator().manual_seed(1))


def same_batch(a, b):
    assert torch.equal(a.x, b.x) and torch.equal(a.y, b.y)
    for la, lb in zip(a.multiscale, b.multiscale):
        for name in ('pos', 'neighbor_idx', 'sub_idx', 'up_idx'):
            u, v = getattr(la, name), getattr(lb, name)
            assert (u is None and v is None) or torch.equal(u, v), name


def test_identity_augmentation_changes_nothing():
    from crfconv_amd.data import CollateGraph
    B, N = 2, 4096
    identity = T.Compose([T.RandomRotate(0, axis=2), T.RandomScaleAnisotropic([1, 1]), T.RandomNoise(sigma=0), T.DropFeature(0),
                          T.AddFeatsByKeys([True, True], ['pos', 'rgb'], delete_feats=[False, True])],
                         generator=torch.Generator().manual_seed(5))
    plain_t, aug_t = static_batch(B, N), static_batch(B, N)
    plain = CollateGraph(plain_t, generator=torch.Generator().manual_seed(7))
    aug = CollateGraph(aug_t, generator=torch.Generator().manual_seed(7), augment=identity)
    assert plain.seed == aug.seed                         # the augmentation costs no generator draw
    for seed in (510, 520):
        pos, x, y = clouds(seed, B, N)
        plain.run(pos, x, y)
        aug.run(pos, x, y)
        same_batch(aug_t, plain_t)
        assert all(torch.equal(u, v) for u, v in zip(plain.choices, aug.choices))


def test_knn_sees_the_augmented_coordinates():
    import crfconv_amd
    from crfconv_amd.data import CollateGraph
    B, N = 2, 4096
    chain = train_chain(sigma=0.0)                       # noise-free: the restatement needs no per-point draws
    static = static_batch(B, N)
    cg = CollateGraph(static, generator=torch.Generator().manual_seed(8), augment=chain)
    pos, x, y = clouds(530, B, N)
    cg.run(pos, x, y)
    assert cg.state_dict()['counter'] == 1
    pout = torch.empty((B, 8), device=DEV)                # the parameters the graph applied: the same (seed, counter) again
    chain.apply_batch(pos.clone(), x.clone(), cg.seed, cg.counter, params_out=pout)
    params = pout.cpu().numpy()
    np.testing.assert_array_equal(params[:, 5:7], chain.draws(cg.seed, 1, B)['params'][:, 5:7])
    want_pos, want_x, _ = restate(pos.cpu().numpy(), x[..., 3:].cpu().numpy(), params, None, use_noise=False)
    ref = crfconv_amd.multiscale_compute(t(want_pos), x=t(want_x), y=y, choices=[c.clone() for c in cg.choices], sort='morton',
                                         order=cg.order.clone())
    assert torch.equal(crfconv_amd.data.morton_order(t(want_pos)), cg.order)
    same_batch(static, ref)
    assert torch.equal(static.x[..., :3], static.multiscale[0].pos)


def test_replays_resume_and_pipeline():
    from crfconv_amd.data import CollateGraph, CollatePipeline
    B, N = 2, 4096
    chain = train_chain()
    static, static2 = static_batch(B, N), static_batch(B, N)
    cg = CollateGraph(static, generator=torch.Generator().manual_seed(9), augment=chain)
    pos, x, y = clouds(540, B, N)
    cg.run(pos, x, y)
    first = static.multiscale[0].pos.clone()
    cg.run(pos, x, y)                                    # the same clouds again: new parameters, new noise
    assert cg.state_dict()['counter'] == 2
    assert not torch.equal(first, static.multiscale[0].pos)
    assert torch.equal(static.x[..., :3], static.multiscale[0].pos)
    sd = cg.state_dict()
    other = CollateGraph(static2, generator=torch.Generator().manual_seed(10), augment=train_chain(torch.Generator().manual_seed(3)))
    other.load_state_dict(sd)
    pos, x, y = clouds(550, B, N)
    cg.run(pos, x, y)
    other.run(pos, x, y)
    same_batch(static2, static)
    # a pipeline: both slots augment, each from its own graph's seed
    statics = [static_batch(B, N, 600 + k) for k in range(2)]
    pipe = CollatePipeline(statics, generator=torch.Generator().manual_seed(3), augment=chain)
    inputs = [clouds(700 + 10 * i, B, N) for i in range(2)]
    for s in range(2):
        pipe.submit(s, *inputs[s])
    for s in range(2):
        batch = pipe.acquire(s)
        p0 = batch.multiscale[0].pos
        assert torch.equal(batch.x[..., :3], p0)
        zin = inputs[s][0][..., 2].sort(dim=1).values
        assert not torch.allclose(p0[..., 2].sort(dim=1).values, zin)         # z was scaled (and jittered)
        pipe.release(s)
    assert [g.state_dict()['counter'] for g in pipe.graphs] == [1, 1]


def test_per_crop_use_on_the_sampler():
    from crfconv_amd.sampling import PossibilitySampler
    pts = S.make_cloud(31, 20000, box=(10, 10, 3))
    rgb = S.uniform(31, 'rgb', (20000, 3), 0, 1)
    smp = PossibilitySampler([t(pts)], rgb=[t(rgb)], num_points=2048, split='test', generator=torch.Generator().manual_seed(2))
    chain = train_chain()
    data = smp.get_random()
    before = data.pos.clone()
    out = chain(data)
    assert out is data
    assert data.x.shape == (2048, 6) and not hasattr(data, 'rgb')
    assert torch.equal(data.x[:, :3], data.pos)
    assert not torch.equal(data.pos, before)
    assert chain.state_dict()['counter'] == 1
    # a lone transform is a Compose of one
    data = smp.get_random()
    before = data.pos.clone()
    T.RandomNoise(sigma=0.01)(data)
    d = (data.pos - before).abs()
    assert float(d.max()) <= 0.05 + 1e-5 and float(d.max()) > 0 and data.rgb.shape == (2048, 3)


def test_training_step_on_augmented_fresh_batches():
    import torch.nn.functional as F
    from crfconv_amd import models
    from crfconv_amd.data import CollateGraph
    from crfconv_amd.train import GraphedModel
    B, N = 2, 8192
    static = static_batch(B, N)
    torch.manual_seed(6)
    net = GraphedModel(models.PointConvBig(6, 13, True, 3).to(DEV).train())
    opt = torch.optim.SGD(net.parameters(), lr=1e-2, momentum=0.95)
    cg = CollateGraph(static, generator=torch.Generator().manual_seed(11), augment=train_chain())
    for i in range(3):
        cg.collate(*clouds(800 + 10 * i, B, N))
        cg.load()
        assert torch.equal(static.x[..., :3], static.multiscale[0].pos)
        opt.zero_grad()
        loss = F.cross_entropy(net(static), static.y.reshape(-1) - 1, ignore_index=-1)
        loss.backward()
        opt.step()
        assert torch.isfinite(loss).item()
    assert net.fwd_graph is not None and cg.state_dict()['counter'] == 3
