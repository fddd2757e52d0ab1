"""-m gpu: kNN interpolation as one HIP launch and its transpose (csrc/interp.hip, ops.interpolate / ops.knn_interpolate,
models.knn_interpolate) against float64 on the same table; bit-reproducible forward and gradient; the ragged batch equals its clouds run
alone; the wiring of the model-side function; a captured forward replayed over another split.

Inputs: a ragged batch of clouds with 700, 300, 9, 2048, 40 and 2 target points; a quarter of that many sources per cloud (rounded up: the
2-point cloud has ONE source, so its rows hold -1 at k = 3; the 9-point cloud has exactly k), drawn independently in the cloud's box; one
source moved onto a target (d^2 = 0: the clamp); one extra source 100 units away in cloud 0 (nobody's neighbour: in-degree 0).  Features
and upstream gradients are uniform in [0.5, 1.5]: nothing cancels, so every bound is relative per element."""
import numpy as np
import pytest
import torch

import _seeded as S

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SIZES = [700, 300, 9, 2048, 40, 2]
K = 3
CLAMP = float(np.float32(1e-16))          # the kernel's constant is the float32 1e-16f


def make_batch(sizes, seed, far=True):
    """-> pos_x, pos_y (float32 numpy), per-cloud source and target counts."""
    px, py, nx = [], [], []
    for s, n in enumerate(sizes):
        shift = np.float32(3.0 * s)
        tgt = S.make_cloud(seed + s, n, box=(2, 1, 1)) + shift
        src = S.make_cloud(seed + 50 + s, -(-n // 4), box=(2, 1, 1)) + shift
        if s == 0:
            src[5] = tgt[11]                                  # a source ON a target
            if far:
                src = np.concatenate([src, tgt[:1] + np.float32(100.0)])
        px.append(src)
        py.append(tgt)
        nx.append(len(src))
    return np.concatenate(px).astype(np.float32), np.concatenate(py).astype(np.float32), nx, list(sizes)


def dev_ptr(counts):
    return torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)).to(DEV)


def ids_of(counts):
    return torch.from_numpy(np.repeat(np.arange(len(counts)), counts).astype(np.int64)).to(DEV)


def table_case(px, py, nx, ny, k):
    """The segmented search's int32 table over the batch and, in float64 on the same table, the normalised weights and in-degrees."""
    from crfconv_amd.graph import table_from_index
    from crfconv_amd.utils import nearest_neighbors as nn_
    pos_x, pos_y = torch.from_numpy(px).to(DEV), torch.from_numpy(py).to(DEV)
    idx = nn_.knn_segments_device(pos_x, dev_ptr(nx), pos_y, dev_ptr(ny), k, out_dtype=torch.int32)
    tab = idx.cpu().numpy().astype(np.int64)
    valid = tab >= 0
    j = np.where(valid, tab, 0)
    d2 = ((py.astype(np.float64)[:, None, :] - px.astype(np.float64)[j]) ** 2).sum(-1)
    w = np.where(valid, 1.0 / np.maximum(d2, CLAMP), 0.0)
    coef = w / w.sum(1, keepdims=True)
    deg = np.bincount(tab[valid], minlength=len(px))
    return dict(pos_x=pos_x, pos_y=pos_y, nx=nx, ny=ny, tab=tab, table=table_from_index(idx, len(px)), j=j, valid=valid, d2=d2, coef=coef,
                deg=deg, cache={})


@pytest.fixture(scope='module')
def batch():
    px, py, nx, ny = make_batch(SIZES, 900)
    b = table_case(px, py, nx, ny, K)
    tab, deg, far = b['tab'], b['deg'], nx[0] - 1
    assert (tab[-2:, 1:] == -1).all() and (tab[-2:, 0] == len(px) - 1).all()          # the one-source cloud: -1 columns
    assert (tab[:-2] >= 0).all() and not (tab == far).any()                             # the far source is nobody's neighbour
    assert b['d2'][11].min() == 0.0                                                     # the coincident pair is in the table
    print('in-degree: median %d, max %d, zero rows %d' % (np.median(deg), deg.max(), (deg == 0).sum()))
    assert deg[far] == 0
    return b


def case(batch, C):
    """Features, upstream gradient, the HIP result and gradient, and the float64 reference of both, once per table and C."""
    from crfconv_amd import ops
    if C not in batch['cache']:
        n_x, n_y = batch['pos_x'].shape[0], batch['pos_y'].shape[0]
        xn, gn = S.uniform(901, 'x%d' % C, (n_x, C), 0.5, 1.5), S.uniform(901, 'g%d' % C, (n_y, C), 0.5, 1.5)
        x, g = torch.from_numpy(xn).to(DEV).requires_grad_(), torch.from_numpy(gn).to(DEV)
        out = ops.interpolate(x, batch['pos_x'], batch['pos_y'], batch['table'])
        out.backward(g)
        coef, j = batch['coef'], batch['j']
        want = np.einsum('ik,ikc->ic', coef, xn.astype(np.float64)[j])
        dwant = np.zeros((n_x, C))
        contrib = coef[:, :, None] * gn.astype(np.float64)[:, None, :]
        np.add.at(dwant, j[batch['valid']], contrib[batch['valid']])
        batch['cache'][C] = dict(x=x, g=g, out=out.detach(), dx=x.grad.clone(), want=want, dwant=dwant)
    return batch['cache'][C]


# ------------------------------------------------------------------ 1. forward against float64
@pytest.mark.parametrize('C', [8, 5, 64, 512])
def test_forward_against_float64(batch, C):
    """Relative error <= 1e-6, the project's bound for this operator (test_knn_interpolate_on_the_segmented_search); a float32 numpy
    rehearsal in the kernel's order gave 2.4e-7 on these sizes."""
    c = case(batch, C)
    got = c['out'].cpu().numpy()
    assert got.shape == c['want'].shape and got.dtype == np.float32
    err = np.abs(got - c['want']) / np.abs(c['want'])
    print('interpolate forward C=%d: max relative error %.3e' % (C, err.max()))
    assert err.max() <= 1e-6
    on = np.abs(got[11] - c['x'].detach().cpu().numpy()[5].astype(np.float64)) / got[11]
    assert on.max() <= 2.0 ** -22                            # on the coincident source (w = 1e16) the blend is that source's row


# ------------------------------------------------------------------ 2. backward against float64
@pytest.mark.parametrize('C', [8, 5, 64, 512])
def test_backward_against_float64(batch, C):
    """Source row j of in-degree deg_j: relative error <= (8 + deg_j) 2^-24 -- 8 for the roundings of one coefficient and its product,
    deg_j for the sequential sum (the rehearsal stayed below 0.21 of it, largest degree 29).  Rows of in-degree 0 are exactly zero."""
    c = case(batch, C)
    got, want, deg = c['dx'].cpu().numpy(), c['dwant'], batch['deg']
    assert got.shape == want.shape
    assert (got[deg == 0] == 0).all() and (deg == 0).any()
    has = deg > 0
    rel = np.abs(got[has] - want[has]) / np.abs(want[has])
    ratio = rel / ((8 + deg[has])[:, None] * 2.0 ** -24)
    print('interpolate backward C=%d: worst error / bound %.3f (max in-degree %d)' % (C, ratio.max(), deg.max()))
    assert ratio.max() <= 1.0


@pytest.mark.parametrize('k,C', [(1, 16), (5, 64), (16, 8), (16, 5), (3, 1028), (5, 1030)])
def test_other_k_and_wide_rows_against_float64(k, C):
    """Tables of any K take the kernels that keep K a run-time value (K = 3 has its own), and a row of more than 256 pieces (C = 1028:
    257 float4 pieces; C = 1030: one channel per lane) is walked by its workgroup in several passes: forward and gradient against float64 on the
    3096-target batch of the capture test.  Bounds from the roundings, u = 2^-24, all terms positive: a weight carries at most 6 u (a
    difference 1 u, its square 3 u, the three-term sum 2 u more, the reciprocal 1 u), a K-term sequential sum K u more, a division 1 u:
    out = num / den within (6 + K) + (6 + K) + 1 = (13 + 2 K) u; a coefficient w / den within 6 + (6 + K) + 1 = (13 + K) u, its product
    1 u, the sum over the list deg_j u: (14 + K + deg_j) u."""
    px, py, nx, ny = make_batch([2000, 1000, 96], 920)
    b = table_case(px, py, nx, ny, k)
    assert (b['tab'][-96:, :k] >= 0).all()                   # 24 sources in the small cloud: every slot is filled
    c = case(b, C)
    u = 2.0 ** -24
    err = np.abs(c['out'].cpu().numpy() - c['want']) / c['want']
    has = b['deg'] > 0
    rel = np.abs(c['dx'].cpu().numpy()[has] - c['dwant'][has]) / c['dwant'][has]
    ratio = rel / ((14 + k + b['deg'][has])[:, None] * u)
    print('interpolate K=%d C=%d: forward %.3e (bound %.3e), backward worst error / bound %.3f' % (k, C, err.max(), (13 + 2 * k) * u, ratio.max()))
    assert err.max() <= (13 + 2 * k) * u and ratio.max() <= 1.0
    assert (c['dx'].cpu().numpy()[~has] == 0).all()


# ------------------------------------------------------------------ 3. reproducible
@pytest.mark.parametrize('C', [8, 5])
def test_bit_reproducible_and_equal_to_the_clouds_alone(batch, C):
    from crfconv_amd import ops
    c = case(batch, C)
    pos_x, pos_y, nx, ny = batch['pos_x'], batch['pos_y'], batch['nx'], batch['ny']

    def run(x, px, py, **kw):
        x = x.detach().clone().requires_grad_()
        return x, ops.knn_interpolate(x, px, py, k=K, **kw)
    for _ in range(2):                                       # the same inputs twice: the same bits as the first run
        x, out = run(c['x'], pos_x, pos_y, batch_x=ids_of(nx), batch_y=ids_of(ny))
        out.backward(c['g'])
        assert torch.equal(out, c['out']) and torch.equal(x.grad, c['dx'])
    outs, grads, xo, yo = [], [], 0, 0
    for a, b in zip(nx, ny):                                 # every cloud alone
        x, out = run(c['x'][xo:xo + a], pos_x[xo:xo + a], pos_y[yo:yo + b])
        out.backward(c['g'][yo:yo + b])
        outs.append(out.detach())
        grads.append(x.grad)
        xo, yo = xo + a, yo + b
    assert torch.equal(torch.cat(outs), c['out']) and torch.equal(torch.cat(grads), c['dx'])


# ------------------------------------------------------------------ 4. wiring
def test_model_function_and_pointer_form_agree(batch):
    from crfconv_amd import models, ops
    c = case(batch, 8)
    nx, ny = batch['nx'], batch['ny']
    bx, by = ids_of(nx), ids_of(ny)
    pos_x, pos_y = batch['pos_x'].clone().requires_grad_(), batch['pos_y'].clone().requires_grad_()
    x = c['x'].detach().clone().requires_grad_()
    got = models.knn_interpolate(x, pos_x, pos_y, bx, by, 3)
    got.backward(c['g'])
    assert torch.equal(got, c['out']) and torch.equal(x.grad, c['dx'])
    assert pos_x.grad is None and pos_y.grad is None         # the weights are constants to autograd, as in torch_geometric
    with torch.no_grad():
        assert torch.equal(ops.knn_interpolate(x, pos_x, pos_y, bx, by, 3), c['out'])
        assert torch.equal(ops.knn_interpolate(x, pos_x, pos_y, k=3, ptr_x=dev_ptr(nx), ptr_y=dev_ptr(ny)), c['out'])


def test_cloud_without_sources_gives_zero_rows(batch):
    from crfconv_amd import models, ops
    ny = batch['ny']
    lo, hi = ny[0], ny[0] + ny[1]                            # cloud 1 keeps its targets and loses every source
    nx = [batch['nx'][0], 0] + batch['nx'][2:]
    keep = torch.cat([torch.arange(0, nx[0]), torch.arange(batch['nx'][0] + batch['nx'][1], sum(batch['nx']))]).to(DEV)
    x, pos_x = case(batch, 8)['x'].detach()[keep], batch['pos_x'][keep]
    for fn in (models.knn_interpolate, ops.knn_interpolate):
        out = fn(x, pos_x, batch['pos_y'], ids_of(nx), ids_of(ny), 3)
        assert (out[lo:hi] == 0).all() and (out[:lo] >= 0.5).all() and (out[hi:] >= 0.5).all()
        assert torch.equal(out[:lo], case(batch, 8)['out'][:lo])


# ------------------------------------------------------------------ 5. capture
def test_captured_forward_follows_contents_and_pointers():
    """The ptr form under no_grad in one captured graph; x, both position tensors and both pointer arrays are then overwritten in place
    with another split of the same totals and the graph is replayed once: nothing reached the device through the host."""
    from crfconv_amd import ops
    splits = ([2000, 1000, 96], [96, 1500, 1500])            # sources: 500 + 250 + 24 = 24 + 375 + 375
    sets = []
    for seed, sizes in zip((920, 940), splits):
        px, py, nx, ny = make_batch(sizes, seed, far=False)
        sets.append((torch.from_numpy(S.uniform(seed, 'x', (len(px), 8), 0.5, 1.5)).to(DEV), torch.from_numpy(px).to(DEV),
                     torch.from_numpy(py).to(DEV), dev_ptr(nx), dev_ptr(ny)))
    assert all(a.shape == b.shape for a, b in zip(*sets))
    x, pos_x, pos_y, ptr_x, ptr_y = (t.clone() for t in sets[0])
    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            ops.knn_interpolate(x, pos_x, pos_y, k=K, ptr_x=ptr_x, ptr_y=ptr_y)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = ops.knn_interpolate(x, pos_x, pos_y, k=K, ptr_x=ptr_x, ptr_y=ptr_y)
        for dst, src in zip((x, pos_x, pos_y, ptr_x, ptr_y), sets[1]):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        eager = ops.knn_interpolate(*sets[1][:3], k=K, ptr_x=sets[1][3], ptr_y=sets[1][4])
        assert torch.equal(out, eager) and not torch.equal(eager, ops.knn_interpolate(*sets[0][:3], k=K, ptr_x=sets[0][3], ptr_y=sets[0][4]))
