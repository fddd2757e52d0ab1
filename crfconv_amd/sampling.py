"""The two callers either side of tiled-scene inference, on the device:

* ``PossibilitySampler`` -- the crop sampler of datasets/semantic3d_dataset.py:423-460 (``Semantic3D._get_random``;
  the S3DIS copy is s3dis_dataset.py:338-395): seed = arg-min possibility over clouds and points, Gaussian jitter,
  crop = the ``num_points`` nearest points, possibility += (1 - d / d_max)^2 * class weight.
* ``VoteAccumulator`` -- the running mean of soft-max votes per cloud point and the re-projection arg-max of
  trainval.py:170-214.

The reference does both on the host with sklearn's KDTree and numpy; here the clouds, possibilities and vote tables
stay in HBM and each call enqueues a handful of kernels of libcrfconv_amd.so (csrc/sampler.hip, csrc/evaluate.hip).
"""
import contextlib

import numpy as np
import torch

from . import _lib
from .data import Data
from .graph import ptr, require_gpu, stream_ptr, to_device
from .train import no_autograph


def _ws(nbytes, device):
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=device)


_M64 = 0xFFFFFFFFFFFFFFFF
_SMP_DOMAIN = 0x8CB92BA72F3D8DD7            # csrc/sampler.hip SMP_DOMAIN
_SMP_PERM_SLOT = 8
_SMP_CHOICE_SLOT = 1 << 32                  # csrc/sampler.hip SMP_CHOICE_SLOT: slot (j + 1) 2^32 + t


def _smp_hash(seed, counter, b, slots):
    """csrc/sampler.hip smp_hash(seed, counter, b, slot) for an array of slots: uint64."""
    base = (((int(seed) & _M64) ^ _SMP_DOMAIN) + 0x9E3779B97F4A7C15 * (int(counter) + 1) + int(b) * 0xC2B2AE3D27D4EB4F) & _M64
    with np.errstate(over='ignore'):
        z = np.uint64(base) + np.asarray(slots).astype(np.uint64) * np.uint64(0xD1B54A32D192ED03)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


class PossibilitySampler:
    """points: list of float32 [n_c, 3] CUDA tensors (the sub-sampled clouds); rgb / labels: matching lists or None.

    ``class_weight`` float64 [n_classes] and ``label_to_idx`` (dict raw label -> class id) give the per-point update
    weight of the train / val splits (:443-445); ``split='test'`` uses weight 1 and zero labels (:439-441).
    Possibilities start as ``randn * 1e-3`` (:267) from ``generator``, or from ``possibility`` if given.

    ``form='s3dis'`` is the sampler of datasets/s3dis_dataset.py:343-379 instead: the crop is centred on all three axes, the update's
    distances are those of the float32 centred coordinates, there is no class weight and no label map (both are rejected; labels pass
    through unchanged, whatever the split), and a room of fewer than ``num_points`` points is taken whole and padded to ``num_points``
    rows with as few repeats as possible (:375-377, torch_geometric's ``FixedPoints(num_points, replace=False,
    allow_duplicates=True)``): ``get_random`` and ``get_batch`` always return ``num_points`` rows."""

    def __init__(self, points, rgb=None, labels=None, num_points=65536, class_weight=None, label_to_idx=None,
                 split='train', generator=None, possibility=None, noise_scale=3.5 / 10, form='semantic3d'):
        if form not in ('semantic3d', 's3dis'):
            raise ValueError("PossibilitySampler: form must be 'semantic3d' or 's3dis', not %r" % (form,))
        if form == 's3dis' and class_weight is not None:
            raise ValueError("PossibilitySampler(form='s3dis'): the S3DIS sampler has no class_weight (s3dis_dataset.py:364)")
        if form == 's3dis' and label_to_idx is not None:
            raise ValueError("PossibilitySampler(form='s3dis'): the S3DIS sampler has no label_to_idx (s3dis_dataset.py:360)")
        require_gpu(*points)
        self.form = form
        self.points = [p.float().contiguous() for p in points]
        self.device = self.points[0].device
        self.rgb = rgb
        self.split = split
        self.num_points = int(num_points)
        self.noise_scale = float(noise_scale)
        self.generator = generator
        self.labels = None
        self.point_weight = None
        if form == 's3dis':
            if labels is not None:
                self.labels = [lab.to(self.device).long().contiguous() for lab in labels]
        elif split != 'test' and labels is not None:
            self.labels, self.point_weight = [], []
            cw = torch.as_tensor(np.asarray(class_weight, dtype=np.float64)).to(self.device)
            for lab in labels:
                lab = lab.to(self.device).long()
                if label_to_idx is not None:
                    raw = torch.tensor(sorted(label_to_idx), device=self.device)
                    cls = torch.tensor([label_to_idx[k] for k in sorted(label_to_idx)], device=self.device)
                    lab = cls[torch.searchsorted(raw, lab)]
                self.labels.append(lab)
                self.point_weight.append(cw[lab].contiguous())
        if possibility is not None:
            self.possibility = [torch.as_tensor(p, dtype=torch.float64).to(self.device).contiguous().clone()
                                for p in possibility]
        else:
            self.possibility = [(torch.randn(p.shape[0], dtype=torch.float64, generator=generator) * 1e-3).to(self.device)
                                for p in self.points]
        self._ws_min = _ws(_lib.load().crfconv_argmin_workspace(), self.device)
        self._minv = torch.empty(len(self.points), dtype=torch.float64, device=self.device)
        self._mini = torch.empty(len(self.points), dtype=torch.int64, device=self.device)
        for c in range(len(self.points)):
            self._refresh_min(c)
        self._crop_ws = {}
        self._batch = None                                  # get_batch's device tables, built at its first call
        self._seed = None                                   # get_batch's own seed: ONE draw on the generator, at first need
        self._counter = torch.zeros(1, dtype=torch.int64, device=self.device)      # get_batch calls on the own counter so far

    def _refresh_min(self, c):
        p = self.possibility[c]
        _lib.call('crfconv_argmin_f64', ptr(p), p.numel(), ptr(self._minv[c:]), ptr(self._mini[c:]), ptr(self._ws_min),
                  self._ws_min.numel(), stream_ptr())

    @property
    def min_possibility(self):
        return self._minv.cpu().numpy()

    def get_random(self, noise=None, perm=None, choice=None):
        """One crop.  ``noise`` float64 [3] and ``perm`` int64 [k] override the Gaussian jitter and the shuffle (tests
        feed the reference's draws); otherwise they come from ``self.generator``.  Returns ``Data(pos, rgb, y,
        point_idx, cloud_idx)`` with the reference's field meanings (:453-458), all on the device.

        form='s3dis': ``Data(x = [pos, rgb], pos, y, point_idx, cloud_idx)`` of exactly ``num_points`` rows (s3dis_dataset.py:368-379);
        ``perm`` holds a permutation of ``range(k_c)``, k_c = min(n_c, num_points), in its first k_c entries and ``choice`` int64
        [num_points] the padding of a small room (row t = row choice[t] of the shuffled crop; unused when k_c == num_points)."""
        if self.form == 's3dis':
            return self._get_random_s3dis(noise, perm, choice)
        if choice is not None:
            raise ValueError("get_random(choice=) belongs to form='s3dis'")
        c, k, noise, perm = self._next_crop(noise, perm)
        pts = self.points[c]
        n = pts.shape[0]
        noise = to_device(noise.contiguous(), self.device)
        perm = None if perm is False else to_device(perm.contiguous(), self.device)
        key = (n, k)
        if key not in self._crop_ws:
            self._crop_ws[key] = _ws(_lib.load().crfconv_possibility_crop_workspace(n, k), self.device)
        ws = self._crop_ws[key]
        idx = torch.empty(k, dtype=torch.int64, device=self.device)
        xyz = torch.empty((k, 3), dtype=torch.float32, device=self.device)
        center = torch.empty(3, dtype=torch.float64, device=self.device)
        pw = None if self.point_weight is None else self.point_weight[c]
        _lib.call('crfconv_possibility_crop', ptr(pts), n, k, ptr(self._mini[c:]), ptr(noise), ptr(perm), ptr(pw),
                  ptr(self.possibility[c]), ptr(idx), ptr(xyz), ptr(center), ptr(ws), ws.numel(), stream_ptr())
        self._refresh_min(c)                               # :451
        rgb = None if self.rgb is None else self.rgb[c][idx].float()
        if self.labels is None:
            y = torch.zeros(k, dtype=torch.long, device=self.device)
        else:
            y = self.labels[c][idx]
        out = Data(pos=xyz, rgb=rgb, y=y, point_idx=idx, cloud_idx=torch.tensor([c], dtype=torch.long, device=self.device))
        out.center = center
        out.cloud = c                                        # the same as a host int (VoteAccumulator.update takes it without a device read)
        return out

    @staticmethod
    def _padding(kc, k, randperm):
        """FixedPoints(k, replace=False, allow_duplicates=True) for kc < k rows: ceil(k / kc) permutations end to end, cut to k."""
        return torch.cat([randperm(kc) for _ in range(-(-k // kc))])[:k]

    def _next_crop(self, noise, perm):
        """What get_random decides on the host: the cloud c (:424 -- a device -> host read; none with a single cloud), the crop's row
        count k_c = min(n_c, num_points), and the jitter float64 [3] and the shuffle int64 (``False`` = none), as given or drawn from
        ``self.generator`` in the reference's order."""
        c = 0 if len(self.points) == 1 else int(torch.argmin(self._minv).item())
        kc = min(self.num_points, self.points[c].shape[0])
        if noise is None:
            noise = torch.randn(3, dtype=torch.float64, generator=self.generator) * self.noise_scale
        noise = torch.as_tensor(noise, dtype=torch.float64)
        if perm is None:
            perm = torch.randperm(kc, generator=self.generator)
        if perm is not False:
            perm = torch.as_tensor(perm, dtype=torch.int64)
        return c, kc, noise, perm

    def _get_random_s3dis(self, noise, perm, choice):
        """One S3DIS-form crop = the batch call with B = 1 (the same kernels, so get_batch(B) is B of these by construction of the
        stream order); the draws come from ``self.generator`` in the reference's order: jitter, shuffle, then the padding."""
        c, kc, noise, perm = self._next_crop(noise, perm)
        k = self.num_points
        noise = noise.reshape(1, 3)
        if perm is not False:
            perm = perm.reshape(-1).cpu()
            if perm.numel() < kc:
                raise ValueError('get_random: perm holds %d entries, the crop %d rows' % (perm.numel(), kc))
            perm = torch.cat([perm[:kc], torch.full((k - kc,), -1, dtype=torch.int64)]).reshape(1, k)
        if kc < k:
            if choice is None:
                choice = self._padding(kc, k, lambda n: torch.randperm(n, generator=self.generator))
            choice = torch.as_tensor(choice, dtype=torch.int64).reshape(1, k)
        else:
            choice = None
        d = self.get_batch(1, noise=noise, perm=perm, choice=choice, counter=self._counter)      # (nothing is drawn: the counter stays)
        out = Data(x=None if d.x is None else d.x[0], pos=d.pos[0], y=d.y[0], point_idx=d.point_idx[0], cloud_idx=d.cloud_idx[0])
        out.center = d.center[0]
        out.cloud = c
        return out

    # ---- B crops per call, every decision on the device (csrc/sampler.hip)
    @property
    def seed(self):
        """Seed of get_batch's draws when the caller passes none: one draw on ``generator`` (on data._private_generator() without
        one: the global generator never advances), taken at first need so that get_random's sequence is untouched."""
        if self._seed is None:
            from .data import _private_generator
            g = self.generator if self.generator is not None else _private_generator()
            self._seed = int(torch.randint(0, 2 ** 62, (1,), generator=g, dtype=torch.int64, device=g.device).item())
        return self._seed

    def _batch_tables(self):
        if self._batch is not None:
            return self._batch
        k = self.num_points
        for c, p in enumerate(self.points):
            if p.shape[0] < k and self.form != 's3dis':
                raise ValueError('PossibilitySampler.get_batch: cloud %d holds %d points, fewer than num_points = %d (the batch '
                                 'form has fixed shapes)' % (c, p.shape[0], k))
        rgb = None if self.rgb is None else [to_device(torch.as_tensor(r), self.device).float().contiguous() for r in self.rgb]
        labels = None if self.labels is None else [lab.long().contiguous() for lab in self.labels]
        rows = []
        for c, p in enumerate(self.points):
            rows.append([p.data_ptr(), self.possibility[c].data_ptr(),
                         0 if self.point_weight is None else self.point_weight[c].data_ptr(),
                         0 if labels is None else labels[c].data_ptr(), 0 if rgb is None else rgb[c].data_ptr(), p.shape[0]])
        table = to_device(torch.tensor(rows, dtype=torch.int64), self.device)      # crf_cloud_desc [n_clouds]: six 8-byte words each
        self._batch = {'table': table, 'rgb': rgb, 'labels': labels, 'n_max': max(p.shape[0] for p in self.points),
                       'n_min': min(p.shape[0] for p in self.points), 'ws': {},
                       'keep': [t.data_ptr() for t in self.possibility]}
        return self._batch

    @staticmethod
    def draws(seed, counter, B, k=0, noise_scale=1.0, kc=None):
        """Host twin (numpy) of what get_batch draws at (seed, counter value the call reads): dict of u [B, 3, 2] (the 53-bit uniforms in
        (0, 1]), normal [B, 3] (Box-Muller, float64), noise [B, 3] = normal * noise_scale, and perm [B, k] int64 (stable arg-sort
        of the row hashes).  The uniforms and the permutations are the device's exactly; the normals to a few ulp.

        kc (form='s3dis'): the row count k_c = min(n_c, k) of every crop, B of them.  perm[b] then ranks the first k_c hashes only (its
        tail is -1) and the dict gains choice [B, k] int64, the padding: the identity for k_c == k, else the first k entries of
        ceil(k / k_c) permutations of range(k_c) laid end to end, permutation j the stable arg-sort over t of the upper 32 bits of the
        hash of slot (j + 1) 2^32 + t."""
        k = int(k)
        u = np.empty((B, 3, 2))
        perm = np.full((B, k), -1, np.int64)
        choice = None if kc is None else np.empty((B, k), np.int64)
        if kc is not None and len(kc) != B:
            raise ValueError('draws: kc holds %d row counts for B = %d crops' % (len(kc), B))
        for b in range(B):
            h = _smp_hash(seed, counter, b, np.arange(6))
            u[b] = (((h >> np.uint64(11)) + np.uint64(1)).astype(np.float64) * 2.0 ** -53).reshape(3, 2)
            n = k if kc is None else int(kc[b])
            if not 0 < n <= k and k > 0:
                raise ValueError('draws: kc[%d] = %d outside 1 .. k = %d' % (b, n, k))
            perm[b, :n] = np.argsort(_smp_hash(seed, counter, b, _SMP_PERM_SLOT + np.arange(n, dtype=np.uint64)), kind='stable')
            if kc is not None:
                if n == k:
                    choice[b] = np.arange(k)
                else:
                    blocks = [np.argsort(_smp_hash(seed, counter, b, (j + 1) * _SMP_CHOICE_SLOT + np.arange(n, dtype=np.uint64)) >> np.uint64(32),
                                         kind='stable') for j in range(-(-k // n))]
                    choice[b] = np.concatenate(blocks)[:k]
        normal = np.sqrt(-2.0 * np.log(u[..., 0])) * np.cos(2.0 * np.pi * u[..., 1])
        out = {'u': u, 'normal': normal, 'noise': normal * float(noise_scale), 'perm': perm}
        if kc is not None:
            out['choice'] = choice
        return out

    def get_batch(self, B, out=None, noise=None, perm=None, seed=None, counter=None, return_draws=False, choice=None):
        """B crops as ONE library call (47 launches per crop, no host read, capturable in a hipGraph): what B consecutive
        ``get_random`` calls give -- crop b + 1 sees the possibilities crop b updated, the cloud is chosen per crop on the
        device -- stacked into ``Data(pos [B, k, 3], x [B, k, C] or None, y [B, k], point_idx [B, k], cloud_idx [B, 1],
        center [B, 3])``, bit for bit for the same jitter and shuffle.

        out: a Data whose tensors (pos, and optionally x / y / point_idx / cloud_idx / center) receive the batch -- static outputs
        for a captured graph; x has 3 ([pos]) or 6 ([pos, rgb]) channels.  Without `out`, x = [pos, rgb] when the sampler has colours.
        noise float64 [B, 3] / perm int64 [B, k] (``False`` = identity) override the draws.  The draws are keyed on
        (seed, counter): by default the sampler's own ``seed`` and device counter, which the call advances by one BEFORE drawing;
        an explicit `counter` (one-element int64 device tensor) is read as it is and advanced by its owner (a CollateGraph).
        The seed is a launch scalar: a captured call keeps the seed it was captured with.  return_draws: also returns
        (noise [B, 3], perm [B, k]) as used, on the device.  Every cloud must hold at least num_points points.

        form='s3dis': small clouds are welcome (a room below num_points is taken whole and padded, decided per crop on the device; the
        launch shapes do not depend on which cloud is drawn).  Only the first k_c = min(n_c, k) entries of a `perm` row are read;
        `choice` int64 [B, k] overrides the padding (read for crops with k_c < k only; without it and without a counter-keyed draw
        of its own the call refuses clouds below k).  return_draws gives (data, noise, perm, choice): perm rows end in -1 beyond k_c,
        choice rows are the identity for k_c == k."""
        s3dis = self.form == 's3dis'
        if choice is not None and not s3dis:
            raise ValueError("get_batch(choice=) belongs to form='s3dis'")
        tb = self._batch_tables()
        if tb['keep'] != [t.data_ptr() for t in self.possibility]:
            raise _lib.CrfConvError('PossibilitySampler: the possibility tensors were replaced after the first get_batch '
                                    '(load_state_dict copies into them)')
        B, k, dev = int(B), self.num_points, self.device
        if B <= 0:
            raise ValueError('get_batch: B = %d' % B)

        def given(name, shape, dtype):
            t = None if out is None else getattr(out, name, None)
            if t is None:
                return None
            if not (t.is_cuda and t.dtype == dtype and t.is_contiguous() and tuple(t.shape) == shape):
                raise ValueError('get_batch(out=): %s must be a contiguous %s device tensor of shape %s' % (name, dtype, shape))
            return t
        x = None if out is None else getattr(out, 'x', None)
        if x is not None:
            if x.dim() != 3 or x.shape[-1] not in (3, 6):
                raise ValueError('get_batch(out=): x must be [B, k, 3] or [B, k, 6]')
            if x.shape[-1] == 6 and tb['rgb'] is None:
                raise ValueError('get_batch(out=): x has six channels but the sampler holds no colours')
            x = given('x', (B, k, x.shape[-1]), torch.float32)
        elif out is None and tb['rgb'] is not None:
            x = torch.empty((B, k, 6), dtype=torch.float32, device=dev)
        pos = given('pos', (B, k, 3), torch.float32)
        if pos is None:
            pos = torch.empty((B, k, 3), dtype=torch.float32, device=dev)
        res = {'pos': pos, 'x': x}
        for name, shape, dtype in (('y', (B, k), torch.int64), ('point_idx', (B, k), torch.int64), ('cloud_idx', (B, 1), torch.int64),
                                   ('center', (B, 3), torch.float64)):
            t = given(name, shape, dtype)
            res[name] = t if t is not None else torch.empty(shape, dtype=dtype, device=dev)
        if noise is not None:
            noise = to_device(torch.as_tensor(noise, dtype=torch.float64).contiguous(), dev)
            if tuple(noise.shape) != (B, 3):
                raise ValueError('get_batch: noise must be [B, 3]')
        identity = perm is False
        if perm is not None and not identity:
            perm = to_device(torch.as_tensor(perm, dtype=torch.int64).contiguous(), dev)
            if tuple(perm.shape) != (B, k):
                raise ValueError('get_batch: perm must be [B, k]')
        else:
            perm = None
        if choice is not None:
            choice = to_device(torch.as_tensor(choice, dtype=torch.int64).contiguous(), dev)
            if tuple(choice.shape) != (B, k):
                raise ValueError('get_batch: choice must be [B, k]')
        if counter is None:
            counter = self._counter
            _lib.call('crfconv_add_i64', ptr(counter), 1, 1, stream_ptr())
        elif not (torch.is_tensor(counter) and counter.is_cuda and counter.dtype == torch.int64 and counter.numel() >= 1):
            raise ValueError('get_batch: counter must be an int64 device tensor')
        seed = self.seed if seed is None else int(seed)
        noise_out = perm_out = None
        if return_draws:
            noise_out = torch.empty((B, 3), dtype=torch.float64, device=dev)
            perm_out = torch.arange(k, dtype=torch.int64, device=dev).repeat(B, 1) if identity \
                else torch.empty((B, k), dtype=torch.int64, device=dev)
        choice_out = torch.empty((B, k), dtype=torch.int64, device=dev) if return_draws and s3dis else None
        entry = 'crfconv_possibility_crop_batch_s3dis' if s3dis else 'crfconv_possibility_crop_batch'
        if B not in tb['ws']:
            tb['ws'][B] = _ws(getattr(_lib.load(), entry + '_workspace')(tb['n_max'], k, B), dev)
        ws = tb['ws'][B]
        only_s3dis = lambda *a: a if s3dis else ()      # noqa: E731 -- the three arguments the S3DIS entry has more
        _lib.call(entry, ptr(tb['table']), len(self.points), tb['n_max'], *only_s3dis(tb['n_min']), ptr(self._minv), ptr(self._mini),
                  k, B, seed & _M64, ptr(counter), self.noise_scale, ptr(noise), ptr(perm), 1 if identity else 0, *only_s3dis(ptr(choice)),
                  ptr(pos), ptr(x), 0 if x is None else x.shape[-1], ptr(res['y']), ptr(res['point_idx']), ptr(res['cloud_idx']),
                  ptr(res['center']), ptr(noise_out), None if identity else ptr(perm_out), *only_s3dis(ptr(choice_out)),
                  ptr(ws), ws.numel(), stream_ptr())
        for t in list(res.values()) + list(self.possibility) + [self._minv, self._mini]:      # written by library kernels
            if t is not None:
                torch.autograd.graph.increment_version(t)
        data = Data(pos=pos, x=x, y=res['y'], point_idx=res['point_idx'], cloud_idx=res['cloud_idx'])
        data.center = res['center']
        if return_draws and s3dis:
            return data, noise_out, perm_out, choice_out
        return (data, noise_out, perm_out) if return_draws else data

    def snapshot(self):
        """Device copies of everything a get_batch call changes (possibilities, per-cloud minima, the own counter)."""
        return ([p.clone() for p in self.possibility], self._minv.clone(), self._mini.clone(), self._counter.clone())

    def restore(self, snap):
        """Puts a ``snapshot()`` back, in place (a graph's warm-up pass must not consume crops)."""
        for p, q in zip(self.possibility, snap[0]):
            p.copy_(q)
        self._minv.copy_(snap[1])
        self._mini.copy_(snap[2])
        self._counter.copy_(snap[3])

    def state_dict(self):
        """Seed, counter and possibility tables: what a checkpoint needs to continue the crop sequence."""
        return {'seed': int(self.seed), 'counter': int(self._counter.item()), 'possibility': [p.cpu().clone() for p in self.possibility]}

    def load_state_dict(self, sd):
        if len(sd['possibility']) != len(self.possibility):
            raise ValueError('PossibilitySampler.load_state_dict: %d clouds in the checkpoint, %d here' % (len(sd['possibility']), len(self.possibility)))
        self._seed = int(sd['seed'])
        self._counter.fill_(int(sd['counter']))
        for c, (p, q) in enumerate(zip(self.possibility, sd['possibility'])):
            p.copy_(torch.as_tensor(q, dtype=torch.float64))            # in place: the device table points at these tensors
            self._refresh_min(c)


class VoteAccumulator:
    """``test_probs`` of trainval.py:58 (one float32 [n_c, n_classes] table per cloud, zeros) with the update of
    :186-189 and the projection of :198-203."""

    def __init__(self, cloud_sizes, num_classes, smooth=0.98, device='cuda', track_visits=False, allow_repeats=False):
        """track_visits: count the updates of every point (int32 tables beside the votes) -- what ``merge`` needs when the crops of a
        scene are spread over several accumulators (ranks).
        allow_repeats: the rows of an update may name a point more than once (the padded crops of an S3DIS-form sampler; smooth = 0.95
        is the S3DIS value, trainval.py:220): one int32 table per cloud picks the row that is stored (``update(repeated=)``)."""
        self.num_classes = int(num_classes)
        self.smooth = float(smooth)
        self.test_probs = [torch.zeros((int(n), self.num_classes), dtype=torch.float32, device=device) for n in cloud_sizes]
        self.visits = [torch.zeros(int(n), dtype=torch.int32, device=device) for n in cloud_sizes] if track_visits else None
        self._bad = torch.zeros(1, dtype=torch.int32, device=device)
        self._last = [torch.full((int(n),), -1, dtype=torch.int32, device=device) for n in cloud_sizes] if allow_repeats else None
        self._table = None                                  # update_batch's device table of the tensors above, built at its first call

    def update(self, point_idx, cloud_idx, probs=None, logits=None, repeated=None):
        """point_idx int64 [B, N]; cloud_idx int64 [B] or [B, 1]; probs or logits float32 [B * N, C] (the network's
        output layout).  Samples are applied in batch order, as the reference's ``for b in range(batch_size)``.

        repeated: the rows of a sample may name one point several times; the update then has numpy's meaning of
        ``test_probs[c][p_idx] = s * test_probs[c][p_idx] + (1 - s) * probs`` (trainval.py:256-262): every right-hand side is formed
        from the old row, the last row naming a point is stored, a visit is counted once per point.  None = as the accumulator was built
        (``allow_repeats``); False keeps the kernel for distinct rows, which races on repeats."""
        if repeated is None:
            repeated = self._last is not None
        if repeated and self._last is None:
            raise _lib.CrfConvError('VoteAccumulator.update(repeated=True) needs allow_repeats=True at construction')
        src = probs if probs is not None else logits
        require_gpu(point_idx, src)
        B, N = point_idx.shape
        src = src.reshape(B, N, self.num_classes).float().contiguous()
        point_idx = point_idx.long().contiguous()
        # cloud ids: host ints / a list of them are taken as they are; a device tensor costs one device -> host read per call
        clouds = cloud_idx.reshape(B, -1)[:, 0].tolist() if torch.is_tensor(cloud_idx) else ([int(cloud_idx)] if isinstance(cloud_idx, int) else [int(c) for c in cloud_idx])
        for b in range(B):
            tp = self.test_probs[int(clouds[b])]
            if repeated:
                _lib.call('crfconv_vote_update_repeated', ptr(src[b]) if probs is not None else None,
                          ptr(src[b]) if probs is None else None, ptr(point_idx[b]), N, self.num_classes, self.smooth,
                          ptr(tp), tp.shape[0], ptr(self._bad), None if self.visits is None else ptr(self.visits[int(clouds[b])]),
                          ptr(self._last[int(clouds[b])]), stream_ptr())
            elif self.visits is None:
                _lib.call('crfconv_vote_accumulate', ptr(src[b]) if probs is not None else None,
                          ptr(src[b]) if probs is None else None, ptr(point_idx[b]), N, self.num_classes, self.smooth,
                          ptr(tp), tp.shape[0], ptr(self._bad), stream_ptr())
            else:
                _lib.call('crfconv_vote_accumulate_counted', ptr(src[b]) if probs is not None else None,
                          ptr(src[b]) if probs is None else None, ptr(point_idx[b]), N, self.num_classes, self.smooth,
                          ptr(tp), tp.shape[0], ptr(self._bad), ptr(self.visits[int(clouds[b])]), stream_ptr())

    def _desc_table(self):
        """crf_vote_desc [n_clouds] on the device (four 8-byte words per cloud), built once from the accumulator's own tensors."""
        own = list(self.test_probs) + list(self.visits or []) + list(self._last or [])
        keep = [t.data_ptr() for t in own]
        if self._table is None:
            rows = [[tp.data_ptr(), 0 if self.visits is None else self.visits[c].data_ptr(),
                     0 if self._last is None else self._last[c].data_ptr(), tp.shape[0]] for c, tp in enumerate(self.test_probs)]
            self._table = (to_device(torch.tensor(rows, dtype=torch.int64), self.test_probs[0].device), keep)
        elif self._table[1] != keep:
            raise _lib.CrfConvError('VoteAccumulator: a vote / visit table was replaced after the first update_batch (copy into the '
                                    'existing tensors instead)')
        return self._table[0]

    def update_batch(self, point_idx, cloud_idx, probs=None, logits=None, repeated=None):
        """``update`` for a batch whose cloud ids stay on the device: point_idx int64 [B, N]; cloud_idx an int64 DEVICE tensor [B] or
        [B, 1] (what ``get_batch`` and ``CollateGraph(sampler=)`` deliver); probs or logits float32 [B, N, C] or [B * N, C].  ONE library
        call (crfconv_vote_update_batch), no host read: capturable in a hipGraph, and a replay follows the tensors' contents.  The
        samples are applied in batch order; two samples of one call may name the same cloud and the same points, and the tables are
        those of B per-sample ``update`` calls, bit for bit.  repeated: as ``update``.  A cloud id outside the accumulator skips the
        sample and counts its rows (``check()``)."""
        if repeated is None:
            repeated = self._last is not None
        if repeated and self._last is None:
            raise _lib.CrfConvError('VoteAccumulator.update_batch(repeated=True) needs allow_repeats=True at construction')
        if (probs is None) == (logits is None):
            raise ValueError('update_batch: exactly one of probs and logits')
        if not torch.is_tensor(cloud_idx):
            raise TypeError('update_batch: cloud_idx must be an int64 device tensor (host cloud ids go through update)')
        if not torch.is_tensor(point_idx) or point_idx.dim() != 2:
            raise ValueError('update_batch: point_idx must be [B, N]')
        B, N = point_idx.shape
        if cloud_idx.dtype != torch.int64 or cloud_idx.dim() not in (1, 2) or cloud_idx.shape[0] != B:
            raise ValueError('update_batch: cloud_idx must be int64 [B] or [B, 1] with B = %d, got %s %s' % (B, cloud_idx.dtype, tuple(cloud_idx.shape)))
        src = probs if probs is not None else logits
        if src.numel() != B * N * self.num_classes:
            raise ValueError('update_batch: %s holds %d values, [B, N, C] = [%d, %d, %d]' % ('probs' if probs is not None else 'logits', src.numel(), B, N, self.num_classes))
        require_gpu(point_idx, cloud_idx, src)
        src = src.reshape(B, N, self.num_classes).float().contiguous()
        point_idx = point_idx.long().contiguous()
        table = self._desc_table()
        _lib.call('crfconv_vote_update_batch', ptr(table), len(self.test_probs), ptr(src) if probs is not None else None,
                  ptr(src) if probs is None else None, ptr(point_idx), ptr(cloud_idx), cloud_idx.stride(0), B, N, self.num_classes,
                  self.smooth, ptr(self._bad), 1 if repeated else 0, stream_ptr())
        for t in list(self.test_probs) + list(self.visits or []) + [self._bad]:      # written by library kernels
            torch.autograd.graph.increment_version(t)

    def confusion(self, cloud, labels, proj_idx=None, label_shift=0, out=None):
        """Confusion matrix of one cloud's votes, device int64 [C, C] (rows = ground truth), in one pass over the vote table
        (trainval.py:275-278 / :298-310): the prediction of row i is the first arg-max of test_probs[cloud][proj_idx[i]] (of row i itself
        without proj_idx), its class labels[i] - label_shift; labels outside [0, C) are skipped.  Accumulates into `out` when given."""
        tp = self.test_probs[cloud]
        C = self.num_classes
        if out is None:
            out = torch.zeros((C, C), dtype=torch.int64, device=tp.device)
        elif not (torch.is_tensor(out) and out.dtype == torch.int64 and tuple(out.shape) == (C, C) and out.is_contiguous()):
            raise ValueError('confusion(out=): a contiguous int64 [%d, %d] tensor is needed' % (C, C))
        n_rows = labels.numel()
        if proj_idx is None:
            if n_rows != tp.shape[0]:
                raise ValueError('confusion: %d labels for the %d points of cloud %d (no proj_idx)' % (n_rows, tp.shape[0], cloud))
        elif proj_idx.numel() != n_rows:
            raise ValueError('confusion: %d labels for %d projection indices' % (n_rows, proj_idx.numel()))
        require_gpu(labels, proj_idx, out)
        labels = labels.reshape(-1).long().contiguous()
        proj_idx = None if proj_idx is None else proj_idx.reshape(-1).long().contiguous()
        _lib.call('crfconv_vote_confusion', ptr(tp), tp.shape[0], C, ptr(proj_idx), ptr(labels), n_rows, int(label_shift), ptr(out),
                  ptr(self._bad), stream_ptr())
        torch.autograd.graph.increment_version(out)
        return out

    def scores(self, labels, proj=None, class_proportions=None, label_shift=0):
        """(mean IoU, IoUs [C]) of the votes against `labels` (one tensor per cloud): the confusions of all clouds summed
        (trainval.py:272-281, or :304-315 through `proj`, the list of proj_idx tensors onto the full clouds whose labels are then given),
        with class_proportions the rows rescaled to the right number of points per class (:283), then Trainer._iou_from_confusions
        (:286-287, :316-317).  One host copy of a C x C matrix."""
        from .utils.metrics import iou_from_confusions
        if len(labels) != len(self.test_probs) or (proj is not None and len(proj) != len(self.test_probs)):
            raise ValueError('scores: one label (and proj) tensor per cloud: %d clouds' % len(self.test_probs))
        hist = None
        for c in range(len(self.test_probs)):
            hist = self.confusion(c, labels[c], None if proj is None else proj[c], label_shift=label_shift, out=hist)
        conf = hist.cpu().numpy()
        if class_proportions is not None:
            conf = conf.astype(np.float32)
            conf *= np.expand_dims(class_proportions / (np.sum(conf, axis=1) + 1e-6), 1)
        ious = iou_from_confusions(conf)
        return float(np.mean(ious)), ious

    def fold_(self, later_probs, later_visits):
        """self <- the tables ONE accumulator would hold that applied self's updates first and then those behind `later_probs` /
        `later_visits` (lists like self.test_probs / self.visits): trainval.py:188-189 is a running mean v <- s v + (1 - s) p, and
        n later updates of a point scale what was there by s^n (csrc/evaluate.hip: vote_fold_kernel)."""
        if self.visits is None:
            raise _lib.CrfConvError('VoteAccumulator.fold_ needs track_visits=True on both sides')
        for tp, vi, lp, lv in zip(self.test_probs, self.visits, later_probs, later_visits):
            lp = lp.to(tp.device, torch.float32).contiguous()
            lv = lv.to(tp.device, torch.int32).contiguous()
            if lp.shape != tp.shape or lv.shape != vi.shape:
                raise ValueError('fold_: tables of %s / %s against %s / %s' % (tuple(lp.shape), tuple(lv.shape), tuple(tp.shape), tuple(vi.shape)))
            _lib.call('crfconv_vote_fold', ptr(tp), ptr(vi), ptr(lp), ptr(lv), tp.shape[0], self.num_classes, self.smooth, stream_ptr())

    def merge(self, group=None):
        """Crops of one scene sharded over the ranks of a process group (each rank voted its own crops into its own tables): every rank
        leaves with the SAME merged tables -- those of a single accumulator that saw rank 0's crops first, then rank 1's, ... (the
        reference's update is order-dependent; sharding only fixes this order, it does not change the rule).  One all-gather of the
        tables and the visit counts per cloud, folded in rank order.  No-op without a process group."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
            return self
        if self.visits is None:
            raise _lib.CrfConvError('VoteAccumulator.merge needs track_visits=True')
        world = dist.get_world_size(group)
        on_host = dist.get_backend(group) == 'gloo'            # (gloo moves host tensors; RCCL device tensors)
        for c, (tp, vi) in enumerate(zip(self.test_probs, self.visits)):
            send_p, send_v = (tp.cpu(), vi.cpu()) if on_host else (tp, vi)
            all_p = [torch.empty_like(send_p) for _ in range(world)]
            all_v = [torch.empty_like(send_v) for _ in range(world)]
            dist.all_gather(all_p, send_p, group=group)
            dist.all_gather(all_v, send_v, group=group)
            tp.copy_(all_p[0])
            vi.copy_(all_v[0])
            for r in range(1, world):
                _lib.call('crfconv_vote_fold', ptr(tp), ptr(vi), ptr(all_p[r].to(tp.device).contiguous()),
                          ptr(all_v[r].to(tp.device).contiguous()), tp.shape[0], self.num_classes, self.smooth, stream_ptr())
        return self

    def project(self, cloud, proj_idx, label_offset=1):
        """uint8 labels of the original points: arg-max of the votes of their nearest sub-sampled point, + 1 because
        0 means unlabeled (:201-203)."""
        require_gpu(proj_idx)
        tp = self.test_probs[cloud]
        proj_idx = proj_idx.long().contiguous()
        preds = torch.empty(proj_idx.numel(), dtype=torch.uint8, device=tp.device)
        _lib.call('crfconv_vote_project', ptr(tp), ptr(proj_idx), proj_idx.numel(), self.num_classes, tp.shape[0],
                  int(label_offset), ptr(preds), ptr(self._bad), stream_ptr())
        return preds

    def check(self):
        bad = int(self._bad.item())
        if bad:
            raise IndexError('%d point indices outside their cloud' % bad)


class _GraphedCrops:
    """Collate + eval forward of one crop SHAPE as two hipGraph replays (vote_scene(graphed=True)): the first crop of a shape runs eagerly and
    becomes the static batch; ``data.CollateGraph`` (Morton order, kNN at every scale, counter-based subsets, in-place refresh of the static
    batch's tables) and the captured ``net(static)`` serve every later crop of that shape.  Eagerly a crop is ~250 library launches of
    host-bound Python (4.7 ms of network + 2.5 ms of collate at 65 536 points, K = 32, T = 5); replayed it is their kernel time."""

    def __init__(self, net, first, kernel_size, ratio, generator):
        from .data import CollateGraph
        first.point_idx = first.cloud_idx = None         # (per-crop bookkeeping, not inputs of the network: the caller keeps them)
        self.static = first
        self.cg = CollateGraph(first, kernel_size=kernel_size, ratio=ratio, generator=generator)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side), torch.no_grad(), no_autograph():
            net(first)                                   # warm-up outside the capture (lazily built tables, allocator): THIS batch, launch by launch
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(self.graph):
            self.logits = net(first)

    def run(self, pos, x):
        self.cg.run(pos, x)                              # static batch <- this crop (its own Morton order: self.cg.order)
        self.graph.replay()
        return self.logits, self.cg.order


def vote_scene(sampler, net, votes, n_crops, kernel_size=(16, 16, 16, 16, 16), ratio=(4, 4, 4, 4, 2), rank=0, world=1, generator=None,
               timings=None, graphed=False, on_crop=None, graph_cache=None):
    """The inference loop of trainval.py:170-189 on the device for ``n_crops`` crops of the sampler's clouds: crop (possibility
    sampler) -> ``multiscale_compute`` (kNN at every scale) -> ``net`` (eval, no grad) -> soft-max votes into ``votes``.  One crop per
    batch (B = 1: datasets/semantic3d_dataset.py:453-458 yields single crops; the loader's batch dimension only stacks them).
    Features = [xyz, rgb] as the reference's collate builds them (datasets/semantic3d_dataset.py:507-510).

    world > 1: EVERY rank draws the whole crop sequence (the sampler is cheap and its possibilities must evolve as on one GPU), crop i is
    run through the network by rank i % world only; ``votes.merge()`` afterwards gives every rank the full tables.
    graphed: collate and forward of every crop after the first of its shape as hipGraph replays (_GraphedCrops); the random subsets of the
    coarse levels then come from the collate graph's counter-based draw instead of ``torch.randperm`` (any subset is a valid one).
    graph_cache: a dict the captured graphs are kept in across calls (same net, same crop shapes: further scenes pay no capture).
    timings: a dict that receives the summed milliseconds per stage (host clock around device-synchronised stages: a diagnostic mode --
    it serialises host and device).  on_crop(data, logits, point_idx): called per crop with the collated batch (static buffers when graphed:
    clone what is to be kept), the logits and the crop's point ids in the batch's row order (tests).

    An S3DIS-form sampler (``form='s3dis'``) yields crops of exactly num_points rows with x = [pos, rgb] built; the crop of a small room
    names some points twice, so ``votes`` must have been built with ``allow_repeats=True`` and every update is a repeated-index one."""
    import time
    from .data import multiscale_compute
    dev = sampler.device

    def stage(name, fn):
        if timings is None:
            return fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        timings[name] = timings.get(name, 0.0) + (time.perf_counter() - t0) * 1e3
        return out
    repeated = True if getattr(sampler, 'form', 'semantic3d') == 's3dis' else None
    was_training = net.training
    net.eval()
    graphs = graph_cache if graph_cache is not None else {}
    try:
        for i in range(n_crops):
            crop = stage('sample', sampler.get_random)
            if i % world != rank:
                continue
            pos = crop.pos.unsqueeze(0)
            if repeated:                                                  # (s3dis form: x = [pos, rgb] comes with the crop)
                x = (crop.x if crop.x is not None else torch.cat([crop.pos, torch.zeros_like(crop.pos)], -1)).unsqueeze(0)
            else:
                rgb = crop.rgb if crop.rgb is not None else torch.zeros_like(crop.pos)
                x = torch.cat([crop.pos, rgb], -1).unsqueeze(0)
            shape = tuple(pos.shape)
            if graphed and shape in graphs:
                logits, order = stage('collate+network (replays)', lambda: graphs[shape].run(pos, x))
                data = graphs[shape].static
                point_idx = crop.point_idx[order.reshape(-1)].unsqueeze(0)          # the batch's rows are the crop's points in Morton order
            else:
                data = stage('collate', lambda: multiscale_compute(pos, x=x, point_idx=crop.point_idx.unsqueeze(0), cloud_idx=crop.cloud_idx.reshape(1, 1),
                                                                   kernel_size=kernel_size, ratio=ratio, generator=generator, sort='morton'))
                # (graphed: this batch becomes the static one of the capture below -- its own tables are built here, not a self-captured copy's)
                with torch.no_grad(), (no_autograph() if graphed else contextlib.nullcontext()):
                    logits = stage('network', lambda: net(data))
                # the collate reordered the crop along its Morton curve: point_idx travelled with it (multiscale_compute permutes x, y, point_idx alike)
                point_idx = data.point_idx
                if graphed:
                    votes.update(point_idx, crop.cloud, logits=logits, repeated=repeated)
                    if on_crop is not None:
                        on_crop(data, logits, point_idx)
                    graphs[shape] = _GraphedCrops(net, data, kernel_size, ratio, generator)
                    continue
            stage('vote', lambda: votes.update(point_idx, crop.cloud, logits=logits, repeated=repeated))
            if on_crop is not None:
                on_crop(data, logits, point_idx)
    finally:
        net.train(was_training)
    return votes


class SceneVoter:
    """The inference loop of trainval.py:170-189 / :236-262 for ``batch_size`` crops per forward, replayed: every ``step()`` after the
    first is TWO hipGraph replays and nothing else on the host --

    * ``data.CollateGraph(static, sampler=sampler)``: sample B crops (possibility sampler, the cloud of every crop chosen on the device)
      -> Morton order, kNN at every scale, subsets -> ``load_`` into the static batch, ``point_idx`` / ``cloud_idx`` carried along;
    * one graph of ``net(static)`` (eval, no grad) and ``votes.update_batch(static.point_idx, static.cloud_idx, logits=...)``: the
      vote is library launches on the capturing stream, keyed by the DEVICE cloud ids, so it sits in the same capture.

    The first ``step()`` runs eagerly (``sampler.get_batch(B)`` on the sampler's own seed and counter, ``multiscale_compute(sort='morton')``
    with ``torch.randperm`` subsets from `generator`, forward, ``update_batch``), makes that batch the static one and captures the forward
    + vote graph; the collate graph is captured by the second step (its warm-up puts the sampler's state back: no crop is lost).  Later
    crops are keyed on the collate graph's seed and counter (``self.cg``).  Crops reach the votes in sampler order, sample b of a batch
    before sample b + 1.  The sampler must hold colours (x = [pos, rgb]).  An S3DIS-form sampler needs ``votes`` built with
    ``allow_repeats=True`` and votes with the repeated-index rule, as ``vote_scene`` demands.  ``votes.check()`` is the caller's.

    Crops sharded over ranks stay with ``vote_scene(rank=, world=)`` + ``votes.merge()``: with a process group of more than one rank
    initialised every rank would vote the whole scene, which is refused unless ``allow_replicated=True`` says that this is meant."""

    def __init__(self, sampler, net, votes, batch_size, kernel_size=(16, 16, 16, 16, 16), ratio=(4, 4, 4, 4, 2), generator=None,
                 allow_replicated=False):
        import torch.distributed as dist
        self.B = int(batch_size)
        if self.B < 1:
            raise ValueError('SceneVoter: batch_size = %d' % self.B)
        if len(kernel_size) != len(ratio):
            raise ValueError('SceneVoter: %d kernel sizes for %d ratios' % (len(kernel_size), len(ratio)))
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1 and not allow_replicated:
            raise ValueError('SceneVoter votes the whole scene on every rank; crops sharded over %d ranks are vote_scene(rank=, world=) + '
                             'votes.merge() (allow_replicated=True runs the replicated loop)' % dist.get_world_size())
        self.repeated = True if getattr(sampler, 'form', 'semantic3d') == 's3dis' else None
        if self.repeated and votes._last is None:
            raise _lib.CrfConvError('SceneVoter: an S3DIS-form sampler pads small rooms (repeated rows): VoteAccumulator needs '
                                    'allow_repeats=True at construction')
        if sampler.rgb is None:
            raise ValueError('SceneVoter: the sampler holds no colours (the batch form builds x = [pos, rgb])')
        self.sampler, self.net, self.votes = sampler, net, votes
        self.kernel_size, self.ratio, self.generator = tuple(kernel_size), tuple(ratio), generator
        self.static = self.cg = self.graph = self.logits = None
        self.batches = 0                                  # steps taken so far

    def _first(self):
        from .data import CollateGraph, multiscale_compute
        crops = self.sampler.get_batch(self.B)
        data = multiscale_compute(crops.pos, x=crops.x, point_idx=crops.point_idx, cloud_idx=crops.cloud_idx, kernel_size=self.kernel_size,
                                  ratio=self.ratio, num_scales=len(self.kernel_size), generator=self.generator, sort='morton')
        with torch.no_grad(), no_autograph():              # (this batch becomes the static one: the model must not capture a copy of it itself)
            logits = self.net(data)
        # the collate reordered every crop along its Morton curve: point_idx travelled with it
        self.votes.update_batch(data.point_idx, data.cloud_idx, logits=logits, repeated=self.repeated)
        self.static = data
        self.cg = CollateGraph(data, kernel_size=self.kernel_size, ratio=self.ratio, generator=self.generator, sampler=self.sampler)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side), torch.no_grad(), no_autograph():
            self.net(data)                                # warm-up outside the capture (the forward only: a vote would count)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(self.graph):
            self.logits = self.net(data)
            self.votes.update_batch(data.point_idx, data.cloud_idx, logits=self.logits, repeated=self.repeated)
        return logits

    def _step(self, on_batch):
        if self.graph is None:
            logits = self._first()
        else:
            self.cg.run()                                 # static batch <- the next B crops
            self.graph.replay()                           # forward + votes
            logits = self.logits
        self.batches += 1
        if on_batch is not None:
            on_batch(self.static, logits)

    def step(self, on_batch=None):
        """One batch of B crops into the votes.  on_batch(static_batch, logits): the collated batch (static buffers: clone what is kept)
        and the logits [B * N, C] of this batch."""
        if not self.net.training:
            return self._step(on_batch)
        self.net.eval()
        try:
            return self._step(on_batch)
        finally:
            self.net.train(True)

    def run(self, n_batches=None, until_min_possibility=None, on_batch=None, check_every=32):
        """``step()`` until `n_batches` have run and / or the smallest possibility of the scene has reached `until_min_possibility`
        (the reference's stop rule, trainval.py:192,264: read once per "epoch" of `check_every` batches -- one host read per epoch, never
        one per batch).  Returns the votes."""
        if n_batches is None and until_min_possibility is None:
            raise ValueError('SceneVoter.run: n_batches or until_min_possibility is needed')
        if int(check_every) < 1:
            raise ValueError('SceneVoter.run: check_every = %d' % check_every)
        was_training = self.net.training
        self.net.eval()
        try:
            done = 0
            while n_batches is None or done < n_batches:
                if until_min_possibility is not None and done and done % int(check_every) == 0 \
                        and float(np.min(self.sampler.min_possibility)) >= until_min_possibility:
                    break
                self._step(on_batch)
                done += 1
        finally:
            self.net.train(was_training)
        return self.votes
