#!/usr/bin/env python3
"""Regenerates tests/golden/g12_s3dis_sampler.npz by RUNNING THE REFERENCE's S3DIS crop sampler.

    python tests/golden/make_golden_s3dis.py          # needs the reference checkout (CRFCONV_REFERENCE)

``S3DISRoom._get_random`` (datasets/s3dis_dataset.py:343-379) runs as it is, the way g9_eval runs Semantic3D's: the dataset module's
module-scope imports that the method never touches are empty stubs, ``Data`` is an attribute bag, sklearn's ``KDTree`` is real.
torch_geometric is absent, so ``FixedPoints`` is a stub restating the upstream ``allow_duplicates`` branch
(``choice = torch.cat([torch.randperm(n) for _ in range(ceil(num / n))])[:num]``, applied to every tensor whose first dimension is n and
not 1): parity is UNPINNED at that boundary, like FastBatchNorm1d in make_golden.py.  Only data is written: the clouds, the start
possibilities and, per draw, the noise, the shuffle, the padding choice and everything the method returned or updated.

Three rooms against num_points = 1500: 6000 points, 1000 (padded with 2 permutations) and 400 (padded with 4).  The large room's start
possibilities are shifted up by 8e-4 so that the reference alone visits each small room twice before it turns to the large one.
"""
import math
import sys
import types

import numpy as np
import torch

import make_golden as G
from make_golden import S

K = 1500
SIZES = (6000, 1000, 400)
N_DRAWS = 8


class Bag:
    def __init__(self, **kw):
        self.__dict__.update(kw)


CHOICES = []


class FixedPoints:
    """torch_geometric.transforms.FixedPoints restated for replace=False, allow_duplicates=True (the only use, :377)."""

    def __init__(self, num, replace=True, allow_duplicates=False):
        assert not replace and allow_duplicates
        self.num = num

    def __call__(self, data):
        n = data.pos.size(0)
        choice = torch.cat([torch.randperm(n) for _ in range(math.ceil(self.num / n))], dim=0)[:self.num]
        CHOICES.append(choice.numpy().copy())
        for key, item in list(data.__dict__.items()):
            if 'edge' in key:
                continue
            if torch.is_tensor(item) and item.size(0) == n and item.size(0) != 1:
                setattr(data, key, item[choice])
        return data


def main():
    from sklearn.neighbors import KDTree
    empty = lambda *names: {n: None for n in names}      # noqa: E731
    for parent in ('torch_geometric', 'torch_points_kernels', 'torch_points3d', 'torch_points3d.core', 'torch_points3d.datasets',
                   'torch_points3d.datasets.segmentation'):
        sys.modules.setdefault(parent, types.ModuleType(parent))
    ds = G.import_reference_file('datasets/s3dis_dataset.py', 'ref_s3dis', stubs=[
        ('utils', empty('cpp_subsampling', 'nearest_neighbors', 'read_ply', 'write_ply')),
        ('torch_geometric.data', dict(Data=Bag, Dataset=object, InMemoryDataset=object)),
        ('torch_geometric.transforms', dict(FixedPoints=FixedPoints)),
        ('torch_points_kernels.points_cpu', {}), ('torch_points_kernels.points_cuda', {}),
        ('torch_points3d.core.data_transform', {}),
        ('torch_points3d.datasets.base_dataset', empty('BaseDataset')),
        ('torch_points3d.datasets.batch', empty('SimpleBatch')),
        ('torch_points3d.datasets.multiscale_data', empty('MultiScaleData', 'MultiScaleBatch')),
        ('torch_points3d.datasets.segmentation.s3dis', empty('S3DISOriginalFused', 'S3DISSphere', 'S3DISCylinder')),
        ('torch_points3d.datasets.segmentation.shapenet', empty('ShapeNetDataset')),
    ])
    boxes = ((6.0, 5.0, 3.0), (2.5, 2.0, 3.0), (1.5, 1.2, 3.0))
    clouds = [S.make_cloud(1200 + c, n, box=boxes[c]) for c, n in enumerate(SIZES)]
    labels = [S.integers(12, 'lab%d' % c, (n,), 0, 13) for c, n in enumerate(SIZES)]
    rgb = [S.uniform(12, 'rgb%d' % c, (n, 3), 0, 1) for c, n in enumerate(SIZES)]
    poss0 = [S.uniform(12, 'p%d' % c, (n,), -1, 1).astype(np.float64) * 1e-3 for c, n in enumerate(SIZES)]
    poss0[0] = poss0[0] + 8e-4
    fake = Bag(min_possibility=[float(p.min()) for p in poss0], possibility=[p.copy() for p in poss0],
               input_trees=[KDTree(c, leaf_size=50) for c in clouds], input_rgb=rgb, input_labels=labels, num_points=K)
    out = {}
    np.random.seed(4321)
    torch.manual_seed(4321)
    drawn = []
    for draw in range(N_DRAWS):
        state = np.random.get_state()
        n_choices = len(CHOICES)
        d = ds.S3DISRoom._get_random(fake)
        after = np.random.get_state()
        c = int(d.cloud_idx[0])
        kc = min(SIZES[c], K)
        np.random.set_state(state)
        noise = np.random.normal(scale=3.5 / 10, size=(1, 3))        # the draw _get_random made first (:349)
        shuffle = np.arange(kc)
        np.random.shuffle(shuffle)                                      # ... and its shuffle (:357): query_idx[shuffle] is what it left
        assert all(np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b for a, b in zip(np.random.get_state(), after))
        choice = CHOICES[-1] if len(CHOICES) > n_choices else np.arange(K)
        assert (len(CHOICES) > n_choices) == (kc < K)
        tag = 'd%d_' % draw
        assert d.pos.shape == (K, 3) and d.x.shape == (K, 6) and d.y.shape == (K,) and d.point_idx.shape == (K,)
        out[tag + 'noise'] = noise.reshape(-1)
        out[tag + 'shuffle'] = shuffle.astype(np.int32)
        out[tag + 'choice'] = choice.astype(np.int32)
        out[tag + 'cloud'] = d.cloud_idx.numpy()
        out[tag + 'point_idx'] = d.point_idx.numpy().astype(np.int32)
        out[tag + 'pos'] = d.pos.numpy()
        out[tag + 'x'] = d.x.numpy()
        out[tag + 'y'] = d.y.numpy().astype(np.int16)
        out[tag + 'min_possibility'] = np.array(fake.min_possibility)
        drawn.append(c)
        mult = np.bincount(d.point_idx.numpy(), minlength=SIZES[c])
        print('draw %d: cloud %d, k_c %d, multiplicities %d .. %d' % (draw, c, kc, mult[mult > 0].min(), mult.max()))
    # the condition on the fixture: small rooms and the large one both drawn, one small room twice (its second visit sees the update)
    small = [c for c in drawn if SIZES[c] < K]
    assert len(small) >= 2 and drawn.count(0) >= 2 and any(small.count(c) >= 2 for c in set(small)), drawn
    for c in range(3):
        out['possibility%d' % c] = fake.possibility[c]
        out['cloud%d' % c] = clouds[c]
        out['labels%d' % c] = labels[c].astype(np.int16)
        out['rgb%d' % c] = rgb[c]
        out['poss%d' % c] = poss0[c]
    out['num_points'] = np.array(K)
    G.save('g12_s3dis_sampler.npz', **out)


if __name__ == '__main__':
    torch.set_num_threads(4)
    main()
