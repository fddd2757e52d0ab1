"""numpy restatements for the S3DIS-form tests: ``S3DISRoom._get_random`` (datasets/s3dis_dataset.py:343-379) with the jitter, the
shuffle and the padding choice as inputs, and numpy's repeated-index vote update (trainval.py:256-262).  Written from the reference's
text, operation for operation; test_host_sampler_s3dis.py holds them against the fixture the reference itself produced."""
import numpy as np


class S3DISTwin:
    """The sampler's state on the host: float32 clouds, colours, labels, float64 possibilities and their per-cloud minima."""

    def __init__(self, points, rgb, labels, possibility, num_points):
        self.points = [np.asarray(p, np.float32) for p in points]
        self.rgb = [np.asarray(r) for r in rgb]
        self.labels = [np.asarray(lab) for lab in labels]
        self.possibility = [np.asarray(p, np.float64).copy() for p in possibility]
        self.min_possibility = [float(p.min()) for p in self.possibility]
        self.num_points = int(num_points)

    def next_cloud(self):
        return int(np.argmin(self.min_possibility))                              # :344

    def draw(self, noise, shuffle=None, choice=None):
        """One crop: dict of cloud, k_c, point_idx, pos, x, y (num_points rows each).  shuffle: permutation of range(k_c) (None = nearest
        first); choice [num_points]: the padding of a room below num_points (unused otherwise)."""
        k = self.num_points
        c = self.next_cloud()
        pick = int(np.argmin(self.possibility[c]))                               # :345
        pts = self.points[c].astype(np.float64)                                  # the KD-tree holds float64
        centre = pts[pick] + np.asarray(noise, np.float64).reshape(3)            # :349-350
        kc = min(len(pts), k)
        diff = pts - centre
        key = diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1] + diff[:, 2] * diff[:, 2]
        query = np.argsort(key, kind='stable')[:kc]                              # :352-355 (ties: lower point id)
        if shuffle is not None:
            query = query[np.asarray(shuffle, np.int64)[:kc]]                    # :357
        xyz = (pts[query] - centre).astype(np.float32)                           # :358, :368
        sq = xyz * xyz                                                           # :363, float32 throughout
        dists = (sq[:, 0] + sq[:, 1]) + sq[:, 2]
        delta = np.square(np.float32(1) - dists / np.max(dists))                 # :364
        assert delta.dtype == np.float32
        self.possibility[c][query] += delta                                      # :365
        self.min_possibility[c] = float(np.min(self.possibility[c]))             # :366
        rgb = self.rgb[c][query].astype(np.float32)
        y = self.labels[c][query].astype(np.int64)
        if kc < k:                                                               # :375-377
            ch = np.asarray(choice, np.int64)
            query, xyz, rgb, y = query[ch], xyz[ch], rgb[ch], y[ch]
        return {'cloud': c, 'kc': kc, 'point_idx': query.astype(np.int64), 'pos': xyz, 'x': np.concatenate([xyz, rgb], 1), 'y': y}


def vote_repeated(table, visits, point_idx, probs, smooth):
    """test_probs[c][p_idx] = smooth * test_probs[c][p_idx] + (1 - smooth) * probs, in place, numpy's own fancy assignment: all
    right-hand sides from the old rows, the last row naming a point stored.  visits (or None) += 1 per distinct point."""
    table[point_idx] = smooth * table[point_idx] + (1 - smooth) * probs
    assert table.dtype == np.float32
    if visits is not None:
        visits[np.unique(point_idx)] += 1
