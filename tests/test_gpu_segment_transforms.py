"""-m gpu: the ragged-batch transforms on the device (csrc/augment_segments.hip: crfconv_augment_segments, crfconv_fixed_points)
against the numpy float64 restatement of tests/segment_transforms_restatement.py and the exact host twins of the draws
(transforms.Compose.draws, transforms.FixedPoints.draws), their capture in one graph, and a ShapeNet-Part style training step."""
import ctypes
import re

import numpy as np
import pytest
import torch

import segment_transforms_restatement as R
from gpu_util import DEV, t
from crfconv_amd import _lib
from crfconv_amd import transforms as T
from crfconv_amd.data import Data

pytestmark = pytest.mark.gpu

# starts at every residue mod 4, an empty cloud in the middle, the 4-points-per-lane and the 1024-thread boundaries, one cloud that
# needs two trips of the workgroup
SIZES = [1, 3, 4, 5, 0, 63, 64, 65, 1023, 1024, 1025, 4097]
U = 2.0 ** -24
SENTINEL = -12345.0


class Batch:
    def __init__(self, sizes, seed=0):
        self.sizes = list(sizes)
        self.ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        self.S, self.N = len(sizes), int(self.ptr[-1])
        rng = np.random.default_rng(seed)
        off = rng.uniform(-400, 400, (self.S, 3))                                 # coordinates offset by a few hundred: centring matters
        self.pos = np.concatenate([rng.uniform(-1, 1, (n, 3)) * [3, 2, 1] + off[b] for b, n in enumerate(sizes)]).astype(np.float32)
        nrm = rng.standard_normal((self.N, 3))
        self.norm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
        self.norm[[2, 70, self.N - 1]] = 0                                        # zero normals stay zero
        self.rgb = rng.uniform(0, 1, (self.N, 3)).astype(np.float32)
        self.noise = rng.uniform(-0.1, 0.1, (self.N, 3)).astype(np.float32)      # half of it beyond clip = 0.05
        self.y = np.arange(self.N, dtype=np.int64)
        th = rng.uniform(-np.pi, np.pi, self.S)
        self.params = np.zeros((self.S, 8), np.float32)
        self.params[:, 0], self.params[:, 1] = np.cos(th), np.sin(th)
        self.params[:, 2:5] = rng.uniform(0.8, 1.2, (self.S, 3))
        self.params[:, 5] = np.arange(self.S) % 8
        self.params[:, 6] = np.arange(self.S) % 2


@pytest.fixture(scope='module')
def batch():
    return Batch(SIZES)


def rows(a, lead=0):
    """`a` on the device as rows lead .. of a larger buffer of sentinels: (buffer, view).  lead = 1 moves every cloud's start by 12
    (24 at C = 6) bytes: the 16-byte aligned address falls elsewhere in every lane's rows."""
    buf = torch.full((lead + a.shape[0] + 3, a.shape[1]), SENTINEL, device=DEV)
    view = buf[lead:lead + a.shape[0]]
    view.copy_(t(a))
    assert view.is_contiguous()
    return buf, view


def untouched(buf, lead, n):
    return bool((buf[:lead] == SENTINEL).all() and (buf[lead + n:] == SENTINEL).all())


def full_chain(axis, layout, seed=7):
    steps = [T.NormalizeScale(), T.RandomRotate(180, axis=axis), T.RandomScaleAnisotropic([0.8, 1.2]),
             T.RandomSymmetry([True, True, True]), T.RandomNoise(sigma=0.03, clip=0.05)]
    if layout == 'pos_rgb':
        steps += [T.DropFeature(0.2), T.AddFeatsByKeys([True, True], ['pos', 'rgb'])]
    elif layout == 'pos_norm':
        steps += [T.AddFeatsByKeys([True, True], ['pos', 'norm'])]
    elif layout == 'pos':
        steps += [T.AddFeatsByKeys([True], ['pos'])]
    return T.SegmentCompose(steps, generator=torch.Generator().manual_seed(seed))


def counter0():
    return torch.zeros(1, dtype=torch.int64, device=DEV)


def check_against_restatement(bt, got_pos, got_norm, got_x, pout, sout, ref, n_ops, n_ops_norm):
    """Every element of pos, norm and x, cloud by cloud, within n_ops * 2^-24 * R of the float64 restatement."""
    for b in range(bt.S):
        lo, hi = bt.ptr[b], bt.ptr[b + 1]
        if hi == lo:
            continue
        bound = n_ops * U * ref['R'][b]
        err = np.abs(got_pos[lo:hi].astype(np.float64) - ref['pos'][lo:hi]).max()
        assert err <= bound, ('pos', b, bt.sizes[b], err, bound)
        if got_norm is not None:
            bound_n = n_ops_norm * U * ref['Rn'][b]
            err = np.abs(got_norm[lo:hi].astype(np.float64) - ref['norm'][lo:hi]).max()
            assert err <= bound_n, ('norm', b, bt.sizes[b], err, bound_n)
        if got_x is not None:
            err = np.abs(got_x[lo:hi].astype(np.float64) - ref['x'][lo:hi]).max(0)
            assert err[:3].max() <= bound, ('x[:, 0:3]', b, err, bound)
            if got_x.shape[1] == 6:
                assert err[3:].max() <= (n_ops_norm * U * ref['Rn'][b] if got_norm is not None and ref['Rn'][b] else 0.0), ('x[:, 3:6]', b, err)


@pytest.mark.parametrize('lead', [0, 1])
@pytest.mark.parametrize('layout,axis', [('pos_norm', 2), ('pos_rgb', 0), ('pos', 1), (None, 2)])
def test_given_parameters_and_noise_match_the_restatement(batch, layout, axis, lead):
    bt = batch
    chain = full_chain(axis, layout)
    with_norm = layout in ('pos_norm', None)
    pbuf, pos = rows(bt.pos, lead)
    nbuf, norm = rows(bt.norm, lead) if with_norm else (None, None)
    zbuf, noise = rows(bt.noise, lead)
    xbuf = x = None
    if layout == 'pos_rgb':
        xbuf, x = rows(np.concatenate([bt.pos * 0 + 7, bt.rgb], 1), lead)          # (x[:, 0:3] is written from pos, whatever it held)
    elif layout == 'pos_norm':
        xbuf, x = rows(np.full((bt.N, 6), 7, np.float32), lead)
    elif layout == 'pos':
        xbuf, x = rows(np.full((bt.N, 3), 7, np.float32), lead)
    pout, sout = torch.full((bt.S, 8), -7.0, device=DEV), torch.full((bt.S, 4), -7.0, device=DEV)
    chain.apply_segments(pos, norm, x, t(bt.ptr), 17, counter0(), params_out=pout, stats_out=sout, params_in=t(bt.params), noise_in=noise)
    po, so = pout.cpu().numpy(), sout.cpu().numpy()
    # what was applied: the given parameters, for every cloud (the empty one too)
    want_params = bt.params.copy()
    if layout != 'pos_rgb':
        want_params[:, 6] = 1
    np.testing.assert_array_equal(po[:, :7], want_params[:, :7])
    e = SIZES.index(0)
    np.testing.assert_array_equal(so[e], [0, 0, 0, 0])
    assert po[e, 7] == 0
    ref = R.restate(bt.pos, bt.ptr, po, so, norm=bt.norm if with_norm else None, rgb=bt.rgb if layout == 'pos_rgb' else None,
                    noise=bt.noise, center=True, normalize=True, axis=axis, scale=True, flip_axes=7, clip=float(np.float32(0.05)), drop=True,
                    x_layout=layout)
    # n_ops (positions).  The plain count of float32 roundings on the longest path is 8 (center 1, normalize 1, rotate 3, scale 1, flip 1,
    # noise 1), but 8 * 2^-24 * R is not a bound on the error: a rotation passes on the errors of BOTH its inputs (weights |c| + |s| up
    # to sqrt 2), a scale stretches what came in by up to 1.2, and a flip subtracts from a maximum that carries the same error as the
    # coordinate.  The count below weights each rounding by what the later steps can make of it; R leaves the input itself out (the
    # largest COMPUTED magnitude), which is stricter than counting it.  Each rounding is at most 2^-24 of R:
    #   center 1, normalize 1                                          -> 2
    #   rotate: c x_a -+ s x_b carries (|c| + |s|) <= sqrt(2) of the 2, two products and a sum  -> 2 sqrt(2) + 3 = 5.83
    #   scale: a factor of at most 1.2 on what came in, one product     -> 1.2 * 5.83 + 1 = 8.0
    #   flip: the maximum and the coordinate each carry that, one difference -> 2 * 8.0 + 1 = 17.0
    #   noise: one sum                                                 -> 18
    # n_ops (normals): the rotation's 3 roundings per component (the input is exact), divided by s >= 0.8 -> 3.75; the
    #   renormalisation v / |v| moves a component by at most |error vector| / |v| <= sqrt(3) * 3.75 / (1 / 1.2) = 7.8; the scale
    #   and the renormalisation are computed in double and rounded once -> 9
    n_ops, n_ops_norm = 18, 9
    check_against_restatement(bt, pos.cpu().numpy(), None if norm is None else norm.cpu().numpy(), None if x is None else x.cpu().numpy(),
                              po, so, ref, n_ops, n_ops_norm)
    # the recorded c_max: the maximum the lowest flipped axis was subtracted from (carries the 8 roundings up to the flip)
    for b in range(bt.S):
        flip = int(po[b, 5])
        if bt.sizes[b] and flip:
            i = [i for i in range(3) if (flip >> i) & 1][0]
            assert abs(po[b, 7] - ref['cmax'][b, i]) <= 8 * U * ref['R'][b], (b, po[b, 7], ref['cmax'][b, i])
    # x repeats pos (and norm) bit for bit; a dropped rgb is exactly zero, a kept one untouched
    if x is not None:
        assert torch.equal(x[:, :3], pos)
        if layout == 'pos_norm':
            assert torch.equal(x[:, 3:], norm)
        if layout == 'pos_rgb':
            keep = np.repeat(po[:, 6], bt.sizes).astype(bool)
            np.testing.assert_array_equal(x[:, 3:].cpu().numpy(), bt.rgb * keep[:, None])
            assert 0 < keep.sum() < bt.N
    # the mean as applied lies within one float32 ulp of the float64 mean
    for b in range(bt.S):
        if bt.sizes[b]:
            mean = bt.pos[bt.ptr[b]:bt.ptr[b + 1]].astype(np.float64).mean(0)
            assert np.all(np.abs(so[b, :3] - mean) <= np.spacing(np.abs(mean).astype(np.float32))), (b, so[b, :3], mean)
    # nothing outside the batch's rows was written
    assert untouched(pbuf, lead, bt.N) and (nbuf is None or untouched(nbuf, lead, bt.N)) and (xbuf is None or untouched(xbuf, lead, bt.N))
    assert untouched(zbuf, lead, bt.N) and torch.equal(noise, t(bt.noise))


def test_identity_chains(batch):
    bt = batch
    ptr = t(bt.ptr)
    # Center alone
    pos, norm = t(bt.pos), t(bt.norm)
    sout = torch.full((bt.S, 4), -7.0, device=DEV)
    T.SegmentCompose([T.Center()]).apply_segments(pos, norm, None, ptr, 1, counter0(), stats_out=sout)
    got = pos.cpu().numpy().astype(np.float64)
    assert torch.equal(norm, t(bt.norm))                                           # Center leaves the normals alone
    np.testing.assert_array_equal(sout[:, 3].cpu().numpy(), 1.0)                   # k = 1 without normalize
    for b in range(bt.S):
        lo, hi = bt.ptr[b], bt.ptr[b + 1]
        if hi > lo:
            assert np.abs(got[lo:hi].mean(0)).max() < 2.0 ** -23 * np.abs(bt.pos[lo:hi]).max(), (b, got[lo:hi].mean(0))
    # NormalizeScale
    pos = t(bt.pos)
    T.SegmentCompose([T.NormalizeScale()]).apply_segments(pos, norm, None, ptr, 1, counter0(), stats_out=sout)
    got = pos.cpu().numpy()
    assert torch.equal(norm, t(bt.norm))
    for b in range(bt.S):
        lo, hi = bt.ptr[b], bt.ptr[b + 1]
        if hi - lo > 1:
            assert 0.999998 <= np.abs(got[lo:hi]).max() < 1, (b, np.abs(got[lo:hi]).max())
    one = SIZES.index(1)
    np.testing.assert_array_equal(got[bt.ptr[one]:bt.ptr[one + 1]], 0.0)           # the 1-point cloud: zeros, k = 0 (PyG: NaN)
    assert float(sout[one, 3]) == 0.0
    # coincident points likewise; a lone ``Center()(data)`` works through a SegmentCompose of one
    same = Data(pos=t(np.tile(np.float32([[3.5, -2.25, 100.0]]), (9, 1))), ptr=t(np.array([0, 9], np.int64)))
    assert torch.equal(T.NormalizeScale()(same).pos, torch.zeros(9, 3, device=DEV))
    moved = T.Center()(Data(pos=t(bt.pos[:5]), batch=t(np.array([0, 1, 1, 1, 2], np.int64))))        # (a sorted batch: ptr is rebuilt)
    np.testing.assert_array_equal(moved.ptr.cpu().numpy(), [0, 1, 4, 5])
    np.testing.assert_array_equal(moved.pos[[0, 4]].cpu().numpy(), 0.0)


def test_normals(batch):
    bt = batch
    ptr = t(bt.ptr)
    # unit normals are unit again after an anisotropic scale, within 4 * 2^-24; zero normals stay zero
    chain = T.SegmentCompose([T.RandomRotate(180, axis=1), T.RandomScaleAnisotropic([0.5, 2.0]), T.RandomSymmetry([True, True, True])],
                             generator=torch.Generator().manual_seed(3))
    params = bt.params.copy()
    params[:, 2:5] = np.random.default_rng(1).uniform(0.5, 2.0, (bt.S, 3))
    pos, norm = t(bt.pos), t(bt.norm)
    chain.apply_segments(pos, norm, None, ptr, 5, counter0(), params_in=t(params))
    got = norm.cpu().numpy().astype(np.float64)
    zero = np.all(bt.norm == 0, axis=1)
    assert zero.sum() == 3 and np.all(got[zero] == 0)
    assert np.abs(np.linalg.norm(got[~zero], axis=1) - 1).max() <= 4 * U
    # the normal of a plane a.p = d, transformed, is orthogonal to the transformed in-plane differences
    rng = np.random.default_rng(2)
    a = rng.standard_normal((bt.S, 3))
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    plane, pn = np.zeros((bt.N, 3), np.float32), np.zeros((bt.N, 3), np.float32)
    for b in range(bt.S):
        lo, hi = bt.ptr[b], bt.ptr[b + 1]
        u = np.cross(a[b], [1.0, 0, 0])
        u /= np.linalg.norm(u)
        v = np.cross(a[b], u)
        st = rng.uniform(-2, 2, (hi - lo, 2))
        plane[lo:hi] = st[:, :1] * u + st[:, 1:] * v                               # (in the plane through the origin, to float32 rounding)
        pn[lo:hi] = a[b]
    params[:, 2:5] = rng.uniform(0.8, 1.2, (bt.S, 3))
    pos, norm = t(plane), t(pn)
    pout, sout = torch.zeros((bt.S, 8), device=DEV), torch.zeros((bt.S, 4), device=DEV)
    chain.apply_segments(pos, norm, None, ptr, 5, counter0(), params_in=t(params), params_out=pout, stats_out=sout)
    ref = R.restate(plane, bt.ptr, pout.cpu().numpy(), sout.cpu().numpy(), norm=pn, axis=1, scale=True, flip_axes=7)
    gp, gn = pos.cpu().numpy().astype(np.float64), norm.cpu().numpy().astype(np.float64)
    for b in range(bt.S):
        lo, hi = bt.ptr[b], bt.ptr[b + 1]
        if hi - lo < 2:
            continue
        # positions: rotate 3, scale 1.2 * 3 + 1 = 4.6, flip 2 * 4.6 + 1 -> 11 roundings of R; normals: 9 of Rn (see the test above).
        # A difference of two positions carries twice the position bound per component.  The float32 inputs are not exactly
        # orthogonal: the normal is off by 2^-24 per component, a point off its plane by 2^-24 of its coordinates (<= 2 sqrt(2));
        # the exact chain keeps n.d up to the renormalisation's factor (<= 1.2), with |d before| <= |d after| / 0.8.
        e_p, e_n = 11 * U * ref['R'][b], 9 * U * ref['Rn'][b]
        d = gp[lo + 1:hi] - gp[lo]
        assert np.all(gn[lo:hi] == gn[lo])                                         # one normal per plane, transformed alike
        dot, length = np.abs(d @ gn[lo]), np.linalg.norm(d, axis=1)
        bound = np.sqrt(3) * (2 * e_p + e_n * length) + 1.2 * np.sqrt(3) * U * (length / 0.8 + 2 * 2 * np.sqrt(2))
        assert np.all(dot <= bound), (b, dot.max(), bound.max())
    # a flip negates exactly
    turn = T.SegmentCompose([T.RandomRotate(180, axis=0), T.RandomSymmetry([True, True, True])], generator=torch.Generator().manual_seed(4))
    out = []
    for mask in (0, 7, 2):
        params[:, 5] = mask
        pos, norm = t(bt.pos), t(bt.norm)
        turn.apply_segments(pos, norm, None, ptr, 5, counter0(), params_in=t(params))
        out.append(norm.clone())
    assert torch.equal(out[1], -out[0])
    assert torch.equal(out[2], out[0] * torch.tensor([1.0, -1.0, 1.0], device=DEV))


def test_batch_invariance_and_determinism(batch):
    bt = batch
    chain = full_chain(2, 'pos_norm')

    def run(pos, norm, noise, ptr, params):
        pos, norm = t(pos), t(norm)
        x = torch.empty((pos.shape[0], 6), device=DEV)
        pout, sout = torch.zeros((len(ptr) - 1, 8), device=DEV), torch.zeros((len(ptr) - 1, 4), device=DEV)
        chain.apply_segments(pos, norm, x, t(np.asarray(ptr, np.int64)), 17, counter0(), params_out=pout, stats_out=sout, params_in=t(params),
                             noise_in=t(noise))
        return pos, norm, x, pout, sout
    first = run(bt.pos, bt.norm, bt.noise, bt.ptr, bt.params)
    second = run(bt.pos, bt.norm, bt.noise, bt.ptr, bt.params)
    for a, b in zip(first, second):
        assert torch.equal(a, b)                                                   # two runs: the same bits
    for b in range(bt.S):
        lo, hi = int(bt.ptr[b]), int(bt.ptr[b + 1])
        if hi == lo:
            continue
        alone = run(bt.pos[lo:hi], bt.norm[lo:hi], bt.noise[lo:hi], [0, hi - lo], bt.params[b:b + 1])
        for k, (a, whole) in enumerate(zip(alone, first)):
            part = whole[lo:hi] if k < 3 else whole[b:b + 1]
            assert torch.equal(a, part), (b, bt.sizes[b], k)                       # a cloud run alone: the same bits as inside the batch


def test_drawn_parameters_and_noise(batch):
    bt = batch
    chain = T.SegmentCompose([T.RandomRotate(180, axis=2), T.RandomScaleAnisotropic([0.8, 1.2]), T.RandomSymmetry([True, False, True]),
                              T.RandomNoise(sigma=0.01, clip=0.05), T.DropFeature(0.3), T.AddFeatsByKeys([True, True], ['pos', 'rgb'])],
                             generator=torch.Generator().manual_seed(21))
    dense = T.Compose(list(chain.transforms), generator=torch.Generator().manual_seed(21))
    S = 64
    sizes = [(7 * b) % 50 + 20 for b in range(S)]
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    N = int(ptr[-1])
    pos0 = np.random.default_rng(0).uniform(-1, 1, (N, 3)).astype(np.float32)
    pos, x = t(pos0), t(np.zeros((N, 6), np.float32))
    counter = torch.full((1,), 41, dtype=torch.int64, device=DEV)
    pout, sout = torch.zeros((S, 8), device=DEV), torch.zeros((S, 4), device=DEV)
    chain.apply_segments(pos, None, x, t(ptr), chain.seed, counter, params_out=pout, stats_out=sout)
    got = pout.cpu().numpy()
    host = dense.draws(chain.seed, 41, S)                                          # what Compose predicts for rows 0 .. S - 1
    np.testing.assert_array_equal(got[:, 5], host['flip'])
    np.testing.assert_array_equal(got[:, 6], host['keep'])
    np.testing.assert_allclose(got[:, 2:5], host['scale'], rtol=0, atol=1e-6)
    np.testing.assert_allclose(got[:, 0], host['cos'], rtol=0, atol=1e-6)
    np.testing.assert_allclose(got[:, 1], host['sin'], rtol=0, atol=1e-6)
    assert 0 < host['flip'].astype(bool).sum() < S and 0 < (~host['keep']).sum() < S
    np.testing.assert_array_equal(sout.cpu().numpy(), np.tile(np.float32([0, 0, 0, 1]), (S, 1)))
    # the drawn noise is what separates pos from the restatement without it: inside the clip, not all zero, keyed by the LOCAL row
    ref = R.restate(pos0, ptr, got, sout.cpu().numpy(), axis=2, scale=True, flip_axes=5)
    diff = pos.cpu().numpy() - ref['pos']
    assert np.abs(diff).max() <= 0.05 + 1e-5 and 0.005 < diff.std() < 0.02
    lo, hi = int(ptr[9]), int(ptr[10])
    alone, pa = t(pos0[lo:hi]), torch.zeros((1, 8), device=DEV)
    # cloud 9 alone sits at position 0 of its ptr: given cloud 9's parameters, a point's noise is cloud 0's draw for the same local row
    chain.apply_segments(alone, None, None, t(np.array([0, hi - lo], np.int64)), chain.seed, counter, params_in=t(got[9:10]), params_out=pa)
    lo0, hi0 = int(ptr[0]), int(ptr[1])
    n0 = min(hi0 - lo0, hi - lo)
    noise_alone = alone.cpu().numpy()[:n0] - R.restate(pos0[lo:hi], [0, hi - lo], got[9:10], sout.cpu().numpy()[:1], axis=2, scale=True,
                                                       flip_axes=5)['pos'][:n0]
    np.testing.assert_allclose(noise_alone, diff[lo0:lo0 + n0], rtol=0, atol=4e-6)      # (float32 positions of magnitude 2; the noise is 1e-2)


NONEMPTY = [n for n in SIZES if n]


@pytest.mark.parametrize('num', [1, 64, 2048])
@pytest.mark.parametrize('mode', ['replace', 'subset', 'duplicates'])
def test_fixed_points_equal_the_host_twin(mode, num):
    bt = Batch(NONEMPTY, seed=3)
    fixed = T.FixedPoints(num, replace=mode == 'replace', allow_duplicates=mode == 'duplicates')
    chain = T.SegmentCompose([fixed], generator=torch.Generator().manual_seed(num))
    chain.load_state_dict({'seed': chain.seed, 'counter': 5})
    data = Data(pos=t(bt.pos), norm=t(bt.norm), y=t(bt.y), ptr=t(bt.ptr), category=t(np.arange(bt.S)))
    if mode == 'subset':
        data.sizes = bt.sizes                                                      # (host sizes given: no read of ptr)
    out = chain(data)
    want = fixed.draws(chain.seed, 6, bt.sizes)                                    # the call advanced the counter to 6
    assert chain.state_dict()['counter'] == 6
    idx = want['index']
    np.testing.assert_array_equal(out.y.cpu().numpy(), idx)                        # y = arange: the picks themselves
    np.testing.assert_array_equal(out.pos.cpu().numpy(), bt.pos[idx])
    np.testing.assert_array_equal(out.norm.cpu().numpy(), bt.norm[idx])
    np.testing.assert_array_equal(out.ptr.cpu().numpy(), want['out_ptr'])
    np.testing.assert_array_equal(out.batch.cpu().numpy(), np.repeat(np.arange(bt.S), np.diff(want['out_ptr'])))
    assert out.category.shape == (bt.S,)
    # the launch alone, with the empty cloud in: its picks are -1
    full = Batch(SIZES, seed=3)
    ctr = torch.full((1,), 6, dtype=torch.int64, device=DEV)
    want = fixed.draws(chain.seed, 6, full.sizes)
    got = chain.pick(t(full.ptr), t(want['out_ptr']), full.N, int(want['out_ptr'][-1]), chain.seed, ctr)
    np.testing.assert_array_equal(got.cpu().numpy(), want['index'])
    again = chain.pick(t(full.ptr), t(want['out_ptr']), full.N, int(want['out_ptr'][-1]), chain.seed, ctr)
    assert torch.equal(got, again)


def test_subset_reads_sizes_from_ptr_when_not_given():
    bt = Batch([5, 300, 64], seed=4)
    chain = T.SegmentCompose([T.FixedPoints(64, replace=False)], generator=torch.Generator().manual_seed(8))
    out = chain(Data(pos=t(bt.pos), y=t(bt.y), ptr=t(bt.ptr)))
    want = T.FixedPoints(64, replace=False).draws(chain.seed, 1, bt.sizes)
    np.testing.assert_array_equal(out.y.cpu().numpy(), want['index'])
    np.testing.assert_array_equal(out.ptr.cpu().numpy(), [0, 5, 69, 133])


def test_capture_and_replay(batch):
    bt = Batch(NONEMPTY, seed=5)
    chain = T.SegmentCompose([T.FixedPoints(512), T.NormalizeScale(), T.RandomRotate(180, axis=2), T.RandomNoise()],
                             generator=torch.Generator().manual_seed(13))
    pos, norm, y, ptr = t(bt.pos), t(bt.norm), t(bt.y), t(bt.ptr)
    pout, sout = torch.zeros((bt.S, 8), device=DEV), torch.zeros((bt.S, 4), device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                                  # warm-up: the counter word and out_ptr exist afterwards
        chain(Data(pos=pos, norm=norm, y=y, ptr=ptr), params_out=pout, stats_out=sout)
    torch.cuda.current_stream().wait_stream(side)
    assert chain.state_dict()['counter'] == 1
    graph = torch.cuda.CUDAGraph()
    # one stream and no parallel branches BY CONSTRUCTION: every launch of the call takes graph.stream_ptr(), the current (capturing)
    # stream, and the call records no event and touches no other stream; the assertions below are on what the replay computes
    with torch.cuda.graph(graph):
        out = chain(Data(pos=pos, norm=norm, y=y, ptr=ptr), params_out=pout, stats_out=sout)
    assert chain.state_dict()['counter'] == 1                                      # captured, not run
    assert torch.equal(pos, t(bt.pos)) and torch.equal(norm, t(bt.norm))           # FixedPoints gathers: the inputs stay
    rotate = T.Compose([T.RandomRotate(180, axis=2), T.RandomNoise()], generator=torch.Generator().manual_seed(0))
    seen = []
    for counter in (2, 3):
        graph.replay()
        torch.cuda.synchronize()
        assert chain.state_dict()['counter'] == counter                            # the device counter advanced inside the graph
        want = chain.fixed.draws(chain.seed, counter, bt.sizes)
        np.testing.assert_array_equal(out.y.cpu().numpy(), want['index'])
        np.testing.assert_array_equal(out.ptr.cpu().numpy(), want['out_ptr'])
        host = rotate.draws(chain.seed, counter, bt.S)
        po, so = pout.cpu().numpy(), sout.cpu().numpy()
        np.testing.assert_allclose(po[:, 0], host['cos'], rtol=0, atol=1e-6)
        np.testing.assert_allclose(po[:, 1], host['sin'], rtol=0, atol=1e-6)
        ref = R.restate(bt.pos[want['index']], want['out_ptr'], po, so, norm=bt.norm[want['index']], center=True, normalize=True, axis=2)
        diff = out.pos.cpu().numpy() - ref['pos']                                  # the drawn noise (sigma 0.01, clip 0.05)
        assert np.abs(diff).max() <= 0.05 + 1e-5 and 0.005 < diff.std() < 0.02
        # normals: the rotation's 3 roundings
        assert np.abs(out.norm.cpu().numpy() - ref['norm']).max() <= 3 * U * ref['Rn'].max()
        seen.append((out.y.clone(), pout.clone()))
    assert not torch.equal(seen[0][0], seen[1][0]) and not torch.equal(seen[0][1], seen[1][1])      # a replay draws afresh


def test_shapenet_part_training_step():
    """FixedPoints(512) on three clouds of unequal size, the chain with x = [pos, norm], then CRFSegNet_Part forward and backward."""
    from crfconv_amd import models
    bt = Batch([700, 300, 1000], seed=6)
    chain = T.SegmentCompose([T.FixedPoints(512, replace=False, allow_duplicates=True), T.NormalizeScale(), T.RandomRotate(180, axis=2),
                              T.RandomScaleAnisotropic([0.8, 1.2]), T.RandomSymmetry([True, False, False]), T.RandomNoise(sigma=0.001),
                              T.AddFeatsByKeys([True, True], ['pos', 'norm'])], generator=torch.Generator().manual_seed(2))
    labels = np.random.default_rng(0).integers(0, 4, bt.N)
    data = chain(Data(pos=t(bt.pos), norm=t(bt.norm), y=t(labels), ptr=t(bt.ptr), category=t(np.array([3, 7, 11], np.int64))))
    assert data.pos.shape == (1536, 3) and data.x.shape == (1536, 6) and data.y.shape == (1536,) and data.batch.shape == (1536,)
    assert torch.equal(data.x[:, :3], data.pos) and torch.equal(data.x[:, 3:], data.norm)
    net = models.CRFSegNet_Part(6, n_classes=4).to(DEV).train()
    out = net(data)
    assert out.shape == (1536, 4)
    loss = torch.nn.functional.nll_loss(out, data.y)
    loss.backward()
    assert torch.isfinite(loss)
    for name, p in net.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name


@pytest.mark.parametrize('field,value,fragment', [
    ('rotate_axis', 3, 'rotate_axis=3 outside'),
    ('deg_lo', 200.0, 'rotation range'),                                           # above deg_hi = 180
    ('scale_span', -0.125, 'scale range'),
    ('flip_axes', 8, 'flip_axes=8 outside'),
    ('scale', 2, 'flags must be 0 or 1'), ('noise', 2, 'flags must be 0 or 1'), ('drop', 2, 'flags must be 0 or 1'),
    ('sigma', -1.0, 'noise sigma='),
    ('drop_p', 1.5, 'drop probability'),
])
def test_both_entries_refuse_a_bad_spec_value(field, value, fragment):
    """The spec fields the dense and the ragged record share are checked by one function (csrc/augment_common.hpp: aug_check_spec):
    each bad value is refused by crfconv_augment and by crfconv_augment_segments in the same words, before anything is launched."""
    from crfconv_amd.graph import ptr, stream_ptr
    steps = [T.RandomRotate(180, axis=2), T.RandomScaleAnisotropic([0.8, 1.2]), T.RandomSymmetry([True, False, False]),
             T.RandomNoise(sigma=0.01, clip=0.05), T.DropFeature(0.2)]
    pos, counter, seg = torch.ones((4, 3), device=DEV), counter0(), t(np.array([0, 4], np.int64))
    dense = T.Compose(steps, generator=torch.Generator().manual_seed(1))._spec()
    ragged = T.SegmentCompose(steps, generator=torch.Generator().manual_seed(1))._spec()
    setattr(dense, field, value)
    setattr(ragged, field, value)
    with pytest.raises(_lib.CrfConvError, match=re.escape(fragment)):              # B = 1, N = 4, no x
        _lib.call('crfconv_augment', ptr(pos), None, 1, 4, 0, ctypes.byref(dense), 1, ptr(counter), None, None, None, None, 0, stream_ptr())
    with pytest.raises(_lib.CrfConvError, match=re.escape(fragment)):              # one cloud of 4 rows, no norm, no x
        _lib.call('crfconv_augment_segments', ptr(pos), None, None, 4, 0, ptr(seg), 1, ctypes.byref(ragged), 1, ptr(counter), None, None,
                  None, None, stream_ptr())
    assert torch.equal(pos, torch.ones((4, 3), device=DEV))
