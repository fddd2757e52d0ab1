"""The reference's training augmentation (trainval.py:26-42) on the device: the torch_points3d / torch_geometric transform classes
it composes, with their constructor names and arguments, lowered by ``Compose`` to ONE library call (two with ``RandomSymmetry``):
csrc/augment.hip, ``crfconv_augment``.  A training script swaps its import and keeps trainval.py:26-42 as written::

    from crfconv_amd.transforms import (AddFeatsByKeys, Compose, DropFeature, RandomNoise, RandomRotate,
                                        RandomScaleAnisotropic, RandomSymmetry)

``Compose(...)(data)`` augments one crop (the ``Data`` of ``PossibilitySampler.get_random()``) in place and returns it;
``data.CollateGraph(..., augment=compose)`` runs the same chain on a whole batch inside the captured collate graph, ahead of the
Morton sort and the neighbour tables.

The semantics are restated from the versions the reference targets (torch_geometric 1.x, torch_points3d 1.x); neither library is a
dependency, so parity at this third-party boundary is UNPINNED: no fixture from the real transforms exists.  The draws are not
torch's or Python's ``random`` draws: every parameter is a counter-based hash of (seed, counter, cloud), and any draw from the stated
laws is the reference's semantics.  Supported: any subsequence of RandomRotate -> RandomScaleAnisotropic -> RandomSymmetry ->
RandomNoise -> DropFeature('rgb'), ending with an optional AddFeatsByKeys of 'pos' / 'rgb'; anything else raises
NotImplementedError.  Importing this module, building a ``Compose`` and ``Compose.draws`` need neither a GPU nor the library.

Ragged batches (pos [N, 3] + ptr [S + 1], the sparse networks' input: ShapeNet-Part with normals) go through ``SegmentCompose``
further down: ``FixedPoints``, ``Center`` and ``NormalizeScale`` (torch_geometric's, as trainval.py:10 imports them) ahead of the same
augmentation, with ``data.norm`` carried along; csrc/augment_segments.hip.  ``Compose`` itself still refuses ``data.norm``.
"""
import ctypes

import numpy as np
import torch

_AUG_DOMAIN = 0xA0761D6478BD642F          # csrc/augment.hip: AUG_DOMAIN
_M64 = 0xFFFFFFFFFFFFFFFF


class _Transform:
    """A lone transform applies as a chain of one: a Compose, or a SegmentCompose for a ragged-batch transform."""
    _ragged = False

    def __call__(self, data):
        if getattr(self, '_compose', None) is None:
            self._compose = (SegmentCompose if self._ragged else Compose)([self])
        return self._compose(data)


class RandomRotate(_Transform):
    """torch_geometric.transforms.RandomRotate: theta ~ U(-|degrees|, |degrees|) (or U(*degrees) for a pair) about `axis`,
    pos <- pos @ M with M = [[c, s, 0], [-s, c, 0], [0, 0, 1]] for axis 2 (PyG's matrices for axes 0 and 1)."""

    def __init__(self, degrees, axis=0):
        if isinstance(degrees, (int, float)):
            degrees = (-abs(degrees), abs(degrees))
        if len(degrees) != 2:
            raise ValueError('RandomRotate: degrees must be a number or a (low, high) pair')
        if axis not in (0, 1, 2):
            raise ValueError('RandomRotate: axis must be 0, 1 or 2, got %r' % (axis,))
        self.degrees, self.axis = (float(degrees[0]), float(degrees[1])), int(axis)

    def __repr__(self):
        return 'RandomRotate(%s, axis=%d)' % (self.degrees, self.axis)


class RandomScaleAnisotropic(_Transform):
    """torch_points3d RandomScaleAnisotropic: three independent factors s_i ~ U(scales[0], scales[1]), pos <- pos * s.  The
    `anisotropic` flag is ignored, as it is there."""

    def __init__(self, scales=None, anisotropic=True):
        if scales is None or len(scales) != 2 or not scales[0] <= scales[1]:
            raise ValueError('RandomScaleAnisotropic: scales must be [low, high] with low <= high, got %r' % (scales,))
        self.scales, self.anisotropic = (float(scales[0]), float(scales[1])), anisotropic

    def __repr__(self):
        return 'RandomScaleAnisotropic(scales=%s)' % (list(self.scales),)


class RandomSymmetry(_Transform):
    """torch_points3d RandomSymmetry: for each flagged axis i, with probability 1/2, pos[:, i] <- max(pos[:, i]) - pos[:, i] (the
    max of the crop's current coordinates: after rotation and scaling).  Not a negation."""

    def __init__(self, axis=(False, False, False)):
        if len(axis) != 3:
            raise ValueError('RandomSymmetry: axis must hold three flags, got %r' % (axis,))
        self.axis = [bool(a) for a in axis]

    def __repr__(self):
        return 'RandomSymmetry(axis=%s)' % (self.axis,)


class RandomNoise(_Transform):
    """torch_points3d RandomNoise: pos <- pos + clamp(sigma N(0, 1), -clip, clip), independently per point and axis."""

    def __init__(self, sigma=0.01, clip=0.05):
        if not (sigma >= 0 and clip >= 0):
            raise ValueError('RandomNoise: sigma and clip must be >= 0')
        self.sigma, self.clip = float(sigma), float(clip)

    def __repr__(self):
        return 'RandomNoise(sigma=%g, clip=%g)' % (self.sigma, self.clip)


class DropFeature(_Transform):
    """torch_points3d DropFeature: with probability drop_proba for the whole crop, data[feature_name] <- 0."""

    def __init__(self, drop_proba=0.2, feature_name='rgb'):
        if not 0 <= drop_proba <= 1:
            raise ValueError('DropFeature: drop_proba must lie in [0, 1]')
        self.drop_proba, self.feature_name = float(drop_proba), feature_name

    def __repr__(self):
        return 'DropFeature(drop_proba=%g, feature_name=%r)' % (self.drop_proba, self.feature_name)


class AddFeatsByKeys(_Transform):
    """torch_points3d AddFeatsByKeys: x <- cat of the named features whose flag in list_add_to_x is set, in feat_names order, from
    the AUGMENTED pos; features flagged in delete_feats are removed from the data.  input_nc_feats and stricts are accepted and
    not checked."""

    def __init__(self, list_add_to_x=None, feat_names=None, input_nc_feats=None, stricts=None, delete_feats=None):
        feat_names = list(feat_names or [])
        n = len(feat_names)
        self.feat_names = feat_names
        self.list_add_to_x = [True] * n if list_add_to_x is None else [bool(v) for v in list_add_to_x]
        self.delete_feats = [False] * n if delete_feats is None else [bool(v) for v in delete_feats]
        self.input_nc_feats, self.stricts = input_nc_feats, stricts
        if len(self.list_add_to_x) != n or len(self.delete_feats) != n:
            raise ValueError('AddFeatsByKeys: list_add_to_x, feat_names and delete_feats must have the same length')

    def __repr__(self):
        return 'AddFeatsByKeys(list_add_to_x=%s, feat_names=%s, delete_feats=%s)' % (self.list_add_to_x, self.feat_names,
                                                                                   self.delete_feats)


_ORDER = (RandomRotate, RandomScaleAnisotropic, RandomSymmetry, RandomNoise, DropFeature, AddFeatsByKeys)


def _splitmix(z):
    """The splitmix64 finalizer on a uint64 numpy array (wrapping arithmetic)."""
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _u24(seed, counter, clouds, slot):
    """csrc/augment.hip aug_u24(aug_hash(seed, counter, cloud, slot)) for every cloud: float32 in [0, 1), exact."""
    base = (((int(seed) & _M64) ^ _AUG_DOMAIN) + 0x9E3779B97F4A7C15 * (int(counter) + 1) + int(slot) * 0xD1B54A32D192ED03) & _M64
    with np.errstate(over='ignore'):
        z = np.uint64(base) + clouds.astype(np.uint64) * np.uint64(0xC2B2AE3D27D4EB4F)
        h = _splitmix(z)
    return ((h >> np.uint64(40)).astype(np.float64) * 2.0 ** -24).astype(np.float32)


def _listed(names, last):
    """['a', 'b', 'c'], 'or' -> 'a, b or c'."""
    return names[0] if len(names) == 1 else '%s %s %s' % (', '.join(names[:-1]), last, names[-1])


def _f32_device(t, shape):
    """None, or a contiguous float32 device tensor of that shape."""
    return t is None or (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape)


class Compose:
    """The chain, validated and lowered to one crfconv_augment call.  `generator`: the seed is ONE draw on it at construction (on
    data._private_generator() when None: the global generator never advances); a device counter advances per call.
    ``state_dict()`` / ``load_state_dict()`` carry seed and counter."""

    # what a chain class supplies: the transforms it takes, in their order, and the attribute each lands in; the features
    # AddFeatsByKeys may name and the x it may build; how the messages call the chain and its pos
    _order = _ORDER
    _slots = ('rotate', 'scale', 'symmetry', 'noise', 'drop', 'add')
    _feats = ('pos', 'rgb')
    _layouts = (['pos'], ['pos', 'rgb'])
    _name, _pos_shape = 'Compose', '[k, 3]'

    def __init__(self, transforms, generator=None):
        name = self._name
        flat = []
        for t in transforms:
            flat.extend(t.transforms if isinstance(t, Compose) else [t])
        self.transforms = flat
        for slot in self._slots:
            setattr(self, slot, None)
        last = -1
        for t in flat:
            k = next((i for i, cls in enumerate(self._order) if type(t) is cls), None)
            if k is None:
                raise NotImplementedError('%s: %r is not supported (supported: %s)' % (name, t, ', '.join(c.__name__ for c in self._order)))
            if k <= last:
                raise NotImplementedError('%s: %r out of order; supported is a subsequence of %s'
                                          % (name, t, ' -> '.join(c.__name__ for c in self._order)))
            last = k
            setattr(self, self._slots[k], t)
        if self.drop is not None and self.drop.feature_name != 'rgb':
            raise NotImplementedError('%s: %r: only the rgb feature can be dropped' % (name, self.drop))
        added = None
        if self.add is not None:
            a = self.add
            for feat in a.feat_names:
                if feat not in self._feats:
                    raise NotImplementedError('%s: %r: feature %r (only %s are supported)' % (name, a, feat, _listed(self._feats, 'and')))
            added = [n for n, on in zip(a.feat_names, a.list_add_to_x) if on]
            if added not in self._layouts:
                raise NotImplementedError('%s: %r: x must be %s, got %s'
                                          % (name, a, _listed(['[%s]' % ', '.join(lay) for lay in self._layouts], 'or'), added))
            if any(d for n, d in zip(a.feat_names, a.delete_feats) if n == 'pos'):
                raise NotImplementedError('%s: %r: pos cannot be deleted' % (name, a))
        self.add_rgb, self.add_norm = added == ['pos', 'rgb'], added == ['pos', 'norm']
        if generator is None:
            from .data import _private_generator
            generator = _private_generator()
        self.seed = int(torch.randint(0, 2 ** 62, (1,), generator=generator, dtype=torch.int64, device=generator.device).item())
        self._counter = None                   # device word, made on first use
        self._counter_value = 0

    def __repr__(self):
        return '%s(%s)' % (self._name, ', '.join(repr(t) for t in self.transforms))

    # ---- the kernel's view of the chain
    def _fill_spec(self, s):
        """The fields crf_augment_spec and crf_augment_segments_spec share, written into the record `s`."""
        s.rotate_axis = -1 if self.rotate is None else self.rotate.axis
        s.deg_lo, s.deg_hi = (0.0, 0.0) if self.rotate is None else self.rotate.degrees
        s.scale = 0 if self.scale is None else 1
        lo, span = self._scale_range()
        s.scale_lo, s.scale_span = float(lo), float(span)
        s.flip_axes = self._flip_axes()
        s.noise = 0 if self.noise is None else 1
        s.sigma, s.clip = (0.0, 0.0) if self.noise is None else (self.noise.sigma, self.noise.clip)
        s.drop = 0 if self.drop is None else 1
        s.drop_p = 0.0 if self.drop is None else self.drop.drop_proba
        return s

    def _spec(self):
        from ._lib import AugmentSpec
        return self._fill_spec(AugmentSpec())

    def _scale_range(self):
        if self.scale is None:
            return np.float32(1), np.float32(0)
        lo, hi = np.float32(self.scale.scales[0]), np.float32(self.scale.scales[1])
        return lo, np.float32(hi - lo)

    def _flip_axes(self):
        return 0 if self.symmetry is None else sum(1 << i for i, on in enumerate(self.symmetry.axis) if on)

    def draws(self, seed, counter, B):
        """Host twin of the per-cloud parameter draws of the call with (seed, counter) (csrc/augment.hip aug_cloud_params), numpy:
        dict of u [B, 8] (the uniforms), theta [B] (radians), cos / sin [B], scale [B, 3], flip [B] (mask of the axes flipped),
        keep [B] (bool) and params [B, 8] in the layout of the kernel's params_out (c_max 0).  The uniforms, flip and keep bits and
        scales are the device's exactly; cos / sin to an ulp.  A step the chain does not hold is the identity."""
        clouds = np.arange(int(B), dtype=np.int64)
        u = np.stack([_u24(seed, counter, clouds, k) for k in range(8)], 1)
        theta = np.zeros(B)
        c, s = np.ones(B, np.float32), np.zeros(B, np.float32)
        if self.rotate is not None:
            lo, hi = (float(np.float32(v)) for v in self.rotate.degrees)
            theta = (lo + (hi - lo) * u[:, 0].astype(np.float64)) * 0.017453292519943295
            c, s = np.cos(theta).astype(np.float32), np.sin(theta).astype(np.float32)
        scale = np.ones((B, 3), np.float32)
        if self.scale is not None:
            lo, span = self._scale_range()
            scale = lo + u[:, 1:4] * span
        axes = self._flip_axes()
        flip = np.zeros(B, np.int64)
        for i in range(3):
            if (axes >> i) & 1:
                flip |= (u[:, 4 + i] < np.float32(0.5)).astype(np.int64) << i
        keep = np.ones(B, bool) if self.drop is None else ~(u[:, 7] < np.float32(self.drop.drop_proba))
        params = np.zeros((B, 8), np.float32)
        params[:, 0], params[:, 1], params[:, 2:5], params[:, 5], params[:, 6] = c, s, scale, flip, keep
        return {'u': u, 'theta': theta, 'cos': c, 'sin': s, 'scale': scale, 'flip': flip, 'keep': keep, 'params': params}

    # ---- device
    def apply_batch(self, pos, x, seed, counter, params_out=None, params_in=None, noise_in=None):
        """The chain on B crops at once, in place: pos [B, N, 3] and x [B, N, C] (C in {3, 6}, [pos, rgb]; or None) float32
        contiguous device tensors; x[..., 0:3] receives the augmented pos.  `counter`: one-element int64 device tensor, read by the
        kernel (not advanced here).  params_out [B, 8] float32 records what was applied; params_in [B, 8] / noise_in [B, N, 3]
        replace the draws (tests).  One launch, two with RandomSymmetry; no host synchronisation: capturable."""
        from . import _lib
        from .graph import ptr, stream_ptr

        ok = _f32_device
        if pos.dim() != 3 or pos.shape[-1] != 3:
            raise ValueError('Compose.apply_batch: pos must be [B, N, 3], got %s' % (tuple(pos.shape),))
        B, N, _ = pos.shape
        C = 0 if x is None else x.shape[-1]
        if not ok(pos, (B, N, 3)) or not ok(x, (B, N, C)) or not ok(params_out, (B, 8)) or not ok(params_in, (B, 8)) \
                or not ok(noise_in, (B, N, 3)):
            raise ValueError('Compose.apply_batch: pos [B, N, 3], x [B, N, C], params [B, 8], noise [B, N, 3] must be contiguous '
                             'float32 device tensors')
        if not (counter.is_cuda and counter.dtype == torch.int64):
            raise ValueError('Compose.apply_batch: counter must be an int64 device tensor')
        ws, nbytes = None, 0
        if self._flip_axes():
            nbytes = _lib.load().crfconv_augment_workspace(B, N)
            ws = torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=pos.device)
        _lib.call('crfconv_augment', ptr(pos), ptr(x), B, N, C, ctypes.byref(self._spec()), int(seed) & _M64, ptr(counter),
                  ptr(params_in), ptr(noise_in), ptr(params_out), ptr(ws), nbytes, stream_ptr())
        return pos, x

    # ---- one call on a Data: the steps the two chains share
    def _device_counter(self, device):
        if self._counter is None or self._counter.device != device:
            value = self._counter_value if self._counter is None else int(self._counter.item())
            self._counter = torch.full((1,), value, dtype=torch.int64, device=device)
        return self._counter

    def _advance(self, device):
        """The device counter, one step further: the word this call's draws read."""
        from . import _lib
        from .graph import ptr, stream_ptr
        counter = self._device_counter(device)
        _lib.call('crfconv_add_i64', ptr(counter), 1, 1, stream_ptr())
        return counter

    def _checked_pos(self, data):
        """data.pos as a contiguous float32 device tensor (written back when converted), and what AddFeatsByKeys needs of the data."""
        from .graph import require_gpu
        pos = data.pos
        require_gpu(pos)
        if pos.dim() != 2 or pos.shape[-1] != 3:
            raise ValueError('%s: data.pos must be %s, got %s' % (self._name, self._pos_shape, tuple(pos.shape)))
        if pos.dtype != torch.float32 or not pos.is_contiguous():
            pos = data.pos = pos.float().contiguous()
        for feat, needed in (('rgb', self.add_rgb), ('norm', self.add_norm)):
            if needed and getattr(data, feat, None) is None:
                raise ValueError('%s: %r needs data.%s' % (self._name, self.add, feat))
        if self.add is not None and getattr(data, 'x', None) is not None:
            raise NotImplementedError('%s: %r onto an existing data.x is not supported' % (self._name, self.add))
        return pos

    def _stage_x(self, pos, rgb):
        """The x the kernel fills: [pos, rgb] holds the rgb it may zero, [pos, norm] and [pos] are written whole; None when no step needs one."""
        if self.add_norm:
            return torch.empty((pos.shape[0], 6), dtype=torch.float32, device=pos.device)
        if self.add_rgb or (self.drop is not None and rgb is not None):
            return torch.cat([pos, rgb.to(torch.float32)], -1).contiguous()
        return None if self.add is None else torch.empty_like(pos)

    def _finish(self, data, x):
        """data.rgb after DropFeature, data.x, and the features AddFeatsByKeys deletes."""
        if x is not None and x.shape[-1] == 6 and not self.add_norm:
            data.rgb = x[:, 3:] if self.add is None else x[:, 3:].clone()      # (after DropFeature; x keeps its own copy)
        if self.add is not None:
            data.x = x if (self.add_rgb or self.add_norm) else x[:, :3].contiguous()
            for name, delete in zip(self.add.feat_names, self.add.delete_feats):
                if delete and name in data.__dict__:
                    delattr(data, name)
        return data

    def __call__(self, data, params_out=None):
        """One crop (``Data`` with pos [k, 3] and rgb [k, 3] on the device), augmented in place and returned, as the reference's
        transforms do; with AddFeatsByKeys, data.x = [pos, rgb] [k, C] and the deleted features are gone."""
        if getattr(data, 'norm', None) is not None:
            raise NotImplementedError('Compose: data.norm is not supported (the transforms would rotate it too)')
        pos = self._checked_pos(data)
        x = self._stage_x(pos, getattr(data, 'rgb', None))
        counter = self._advance(pos.device)
        self.apply_batch(pos[None], None if x is None else x[None], self.seed, counter,
                         params_out=None if params_out is None else params_out.view(1, 8))
        return self._finish(data, x)

    def state_dict(self):
        return {'seed': int(self.seed), 'counter': int(self._counter.item()) if self._counter is not None else self._counter_value}

    def load_state_dict(self, sd):
        self.seed = int(sd['seed']) & _M64
        self._counter_value = int(sd['counter'])
        if self._counter is not None:
            self._counter.fill_(self._counter_value)


# ------------------------------------------------------------------------------------------------ ragged batches (pos [N, 3] + ptr)
_FXP_DOMAIN = 0x8CB92BA72F3D8DD7          # csrc/augment_segments.hip: FXP_DOMAIN


class _SegmentTransform(_Transform):
    _ragged = True


class Center(_SegmentTransform):
    """torch_geometric.transforms.Center: pos <- pos - mean(pos), per cloud.  The mean is summed in float64 and rounded once."""

    def __repr__(self):
        return 'Center()'


class NormalizeScale(_SegmentTransform):
    """torch_geometric.transforms.NormalizeScale: centres the cloud, then pos <- pos * (1 / max |pos|) * 0.999999, into (-1, 1).
    A cloud whose centred maximum is 0 (one point, or coincident points) comes out all zero; PyG writes NaN there."""

    def __repr__(self):
        return 'NormalizeScale()'


class FixedPoints(_SegmentTransform):
    """torch_geometric.transforms.FixedPoints per cloud: `num` rows of every cloud, drawn with replacement (replace=True); without
    (replace=False: min(num, n) rows, in ascending row order); or, with allow_duplicates=True, floor(num / n) whole copies of the cloud
    and a subset for the remainder.  The picks are a counter-based hash of (seed, counter, cloud, index), not torch's draws; any draw
    from the stated law is the reference's semantics.  An EMPTY cloud has no row to pick: its picks are -1 and the gather clamps them."""

    def __init__(self, num, replace=True, allow_duplicates=False):
        if int(num) < 1:
            raise ValueError('FixedPoints: num must be >= 1, got %r' % (num,))
        self.num, self.replace, self.allow_duplicates = int(num), bool(replace), bool(allow_duplicates)

    def __repr__(self):
        return 'FixedPoints(%d, replace=%s, allow_duplicates=%s)' % (self.num, self.replace, self.allow_duplicates)

    @property
    def mode(self):
        """The kernel's mode: 0 replace, 1 without replacement, 2 allow_duplicates (replace wins, as in PyG)."""
        return 0 if self.replace else (2 if self.allow_duplicates else 1)

    def counts(self, sizes):
        """Picks per cloud for the cloud sizes `sizes`: num, or min(num, n) without replacement."""
        sizes = np.asarray(sizes, dtype=np.int64)
        return np.minimum(self.num, sizes) if self.mode == 1 else np.full(sizes.shape, self.num, np.int64)

    def draws(self, seed, counter, sizes):
        """Host twin of crfconv_fixed_points for the call with (seed, counter) on clouds of `sizes` rows, numpy, exact: dict of
        index [M] (GLOBAL rows, cloud after cloud; -1 for an empty cloud) and out_ptr [S + 1]."""
        sizes = np.asarray(sizes, dtype=np.int64)
        starts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        out_ptr = np.concatenate([[0], np.cumsum(self.counts(sizes))]).astype(np.int64)
        index = np.full(int(out_ptr[-1]), -1, np.int64)
        mode = self.mode
        for b, n in enumerate(sizes.tolist()):
            m = int(out_ptr[b + 1] - out_ptr[b])
            if m == 0 or n == 0:
                continue
            key = (((int(seed) & _M64) ^ _FXP_DOMAIN) + 0x9E3779B97F4A7C15 * (int(counter) + 1) + b * 0xC2B2AE3D27D4EB4F) & _M64

            def h(count):
                with np.errstate(over='ignore'):
                    return _splitmix(np.uint64(key) + np.arange(count, dtype=np.uint64) * np.uint64(0xD1B54A32D192ED03))
            if mode == 0:
                pick = (((h(m) >> np.uint64(32)) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)
            else:
                whole = (m // n) * n if mode == 2 else 0
                r = min(m - whole, n)
                subset = np.sort(np.argsort(h(n), kind='stable')[:r]).astype(np.int64)      # the r smallest keys, ties to the lower row
                pick = np.concatenate([np.arange(whole, dtype=np.int64) % n, subset])
            index[out_ptr[b]:out_ptr[b] + len(pick)] = starts[b] + pick
        return {'index': index, 'out_ptr': out_ptr}


_ROW_KEYS = ('pos', 'norm', 'rgb', 'x', 'y')           # the per-row attributes FixedPoints gathers; anything else on the data stays as it is


class SegmentCompose(Compose):
    """The chain ahead of the sparse networks on a RAGGED batch (pos [N, 3] + ptr [S + 1]; csrc/augment_segments.hip), validated and
    lowered to a constant number of launches whatever the number of clouds: crfconv_fixed_points + one gather of every row attribute
    (with FixedPoints), then ONE crfconv_augment_segments.  Supported: any subsequence of FixedPoints -> Center | NormalizeScale ->
    RandomRotate -> RandomScaleAnisotropic -> RandomSymmetry -> RandomNoise -> DropFeature('rgb') -> AddFeatsByKeys of 'pos' / 'rgb'
    or 'pos' / 'norm'; anything else raises NotImplementedError.

    data.norm rides along (the library's own semantics; parity with the third-party transforms is unpinned, as for the rest):
    a rotation rotates it, an anisotropic scale s divides it by s and renormalises it to unit length (a zero normal stays zero), a
    flip of axis i negates component i; Center, NormalizeScale and RandomNoise leave it alone.  Cloud b applies the parameters
    ``draws(seed, counter, S)`` predicts for row b, whatever the other clouds hold.

    Seed, device counter, ``state_dict()`` / ``load_state_dict()`` as on ``Compose``; one counter step per call serves the picks and
    the augmentation (two hash domains)."""

    _order = (FixedPoints, Center, NormalizeScale) + _ORDER
    _slots = ('fixed', 'center', 'normalize') + Compose._slots
    _feats = ('pos', 'rgb', 'norm')
    _layouts = (['pos'], ['pos', 'rgb'], ['pos', 'norm'])
    _name, _pos_shape = 'SegmentCompose', '[N, 3]'

    def __init__(self, transforms, generator=None):
        super().__init__(transforms, generator)
        self._out_ptr = {}                     # (S, device) -> arange(S + 1) * num

    def _spec(self):
        from ._lib import AugmentSegmentsSpec
        s = self._fill_spec(AugmentSegmentsSpec())
        s.center = 1 if (self.center is not None or self.normalize is not None) else 0      # NormalizeScale centres first
        s.normalize = 0 if self.normalize is None else 1
        s.x_norm = 1 if self.add_norm else 0
        return s

    def _has_point_step(self):
        return any(getattr(self, slot) is not None for slot in self._slots[1:])

    # ---- device
    def apply_segments(self, pos, norm, x, ptr, seed, counter, params_out=None, stats_out=None, params_in=None, noise_in=None):
        """The chain without FixedPoints on the S clouds of ptr [S + 1] (int64 device tensor), in place: pos [N, 3], norm [N, 3] or
        None, x [N, C] or None (C = 3 [pos]; C = 6 [pos, rgb], or [pos, norm] when AddFeatsByKeys names 'norm'), contiguous float32
        device tensors.  `counter`: one-element int64 device tensor the kernel reads (not advanced here).  params_out [S, 8] and
        stats_out [S, 4] (cx, cy, cz, k) record what was applied; params_in [S, 8] / noise_in [N, 3] replace the draws (tests).
        One launch, no workspace, no host synchronisation: capturable."""
        from . import _lib
        from .graph import ptr as p_, require_gpu, stream_ptr
        if pos.dim() != 2 or pos.shape[-1] != 3:
            raise ValueError('SegmentCompose.apply_segments: pos must be [N, 3], got %s' % (tuple(pos.shape),))
        require_gpu(pos)
        N = pos.shape[0]
        S = ptr.numel() - 1
        C = 0 if x is None else x.shape[-1]
        ok = _f32_device
        if not ok(pos, (N, 3)) or not ok(norm, (N, 3)) or not ok(x, (N, C)) or not ok(params_out, (S, 8)) \
                or not ok(stats_out, (S, 4)) or not ok(params_in, (S, 8)) or not ok(noise_in, (N, 3)):
            raise ValueError('SegmentCompose.apply_segments: pos / norm / noise [N, 3], x [N, C], params [S, 8], stats [S, 4] must be '
                             'contiguous float32 device tensors')
        if not (ptr.is_cuda and ptr.dtype == torch.int64 and ptr.is_contiguous() and ptr.dim() == 1 and S >= 0):
            raise ValueError('SegmentCompose.apply_segments: ptr must be a contiguous int64 device tensor [S + 1]')
        if not (counter.is_cuda and counter.dtype == torch.int64):
            raise ValueError('SegmentCompose.apply_segments: counter must be an int64 device tensor')
        _lib.call('crfconv_augment_segments', p_(pos), p_(norm), p_(x), N, C, p_(ptr), S, ctypes.byref(self._spec()),
                  int(seed) & _M64, p_(counter), p_(params_in), p_(noise_in), p_(params_out), p_(stats_out), stream_ptr())
        return pos, norm, x

    def pick(self, ptr, out_ptr, n_rows, n_picks, seed, counter):
        """crfconv_fixed_points: index [n_picks] int64 GLOBAL rows for the clouds of ptr and the slots of out_ptr (device int64
        [S + 1]); host twin ``FixedPoints.draws``.  One launch, nothing read back."""
        from . import _lib
        from .graph import ptr as p_, stream_ptr
        index = torch.empty(int(n_picks), dtype=torch.int64, device=ptr.device)
        _lib.call('crfconv_fixed_points', p_(ptr), p_(out_ptr), ptr.numel() - 1, int(n_rows), int(n_picks), self.fixed.mode,
                  int(seed) & _M64, p_(counter), p_(index), stream_ptr())
        return index

    def __call__(self, data, params_out=None, stats_out=None):
        """A ragged ``Data``: pos [N, 3], optional norm / rgb [N, 3] and y [N], and ptr [S + 1] (or a SORTED batch [N], which costs
        one host read for S).  Returned transformed: without FixedPoints in place, as the reference's transforms do; with it,
        pos, norm, rgb, x and y (those present) are gathered by the picks, data.ptr / data.batch are rebuilt and every other attribute
        (category, ..) is left as it is; a batch without rows is refused.  With ptr given and FixedPoints absent or in
        the replace / allow_duplicates mode nothing is read back and the call can be captured; replace=False,
        allow_duplicates=False sizes its output by min(num, n): it takes the cloud sizes from data.sizes (host) when present,
        else makes ONE host read of ptr."""
        from .data import pick_rows
        from .graph import to_device
        pos = self._checked_pos(data)
        N, dev = pos.shape[0], pos.device
        seg = getattr(data, 'ptr', None)
        if seg is None:
            batch = getattr(data, 'batch', None)
            if batch is None:
                raise ValueError('SegmentCompose: data needs ptr [S + 1] or a sorted batch [N]')
            S = int(batch[-1].item()) + 1 if N else 0                                        # (the host read of the batch form)
            seg = torch.searchsorted(batch.contiguous(), torch.arange(S + 1, device=dev, dtype=batch.dtype)).to(torch.int64)
        seg = seg.to(torch.int64).contiguous()
        S = seg.numel() - 1
        counter = self._advance(dev)
        if self.fixed is not None:
            if N == 0:
                raise ValueError('SegmentCompose: %r on a batch without rows' % (self.fixed,))
            num = self.fixed.num
            if self.fixed.mode == 1:
                sizes = getattr(data, 'sizes', None)
                if sizes is None:
                    sizes = (seg[1:] - seg[:-1]).cpu()                                        # the ONE documented host read
                counts = self.fixed.counts(np.asarray(sizes, dtype=np.int64))
                out_host = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
                M = int(out_host[-1])
                out_ptr = to_device(torch.from_numpy(out_host), dev)
                batch = torch.repeat_interleave(torch.arange(S, device=dev), to_device(torch.from_numpy(counts), dev), output_size=M)
            else:
                M = S * num
                out_ptr = self._out_ptr.get((S, dev))
                if out_ptr is None:
                    out_ptr = self._out_ptr[(S, dev)] = torch.arange(S + 1, device=dev, dtype=torch.int64) * num
                batch = torch.arange(S, device=dev).view(S, 1).expand(S, num).reshape(-1)
            index = self.pick(seg, out_ptr, N, M, self.seed, counter)
            names = [k for k in _ROW_KEYS if torch.is_tensor(getattr(data, k, None))]
            for k in names:
                if getattr(data, k).shape[0] != N:
                    raise ValueError('SegmentCompose: data.%s has %d rows, data.pos %d' % (k, getattr(data, k).shape[0], N))
            # one launch for all row attributes (B = 1: the picks are global rows)
            moved = pick_rows([getattr(data, k)[None] for k in names], index[None], per_cloud=True)
            for k, m in zip(names, moved):
                setattr(data, k, m[0])
            data.ptr, data.batch = out_ptr.clone(), batch         # (a copy: the caller may edit it, the cached one serves later calls)
            pos, seg = data.pos, out_ptr
        elif getattr(data, 'ptr', None) is None:
            data.ptr = seg
        norm, rgb = getattr(data, 'norm', None), getattr(data, 'rgb', None)
        if norm is not None and (norm.dtype != torch.float32 or not norm.is_contiguous()):
            norm = data.norm = norm.float().contiguous()
        x = self._stage_x(pos, rgb)
        if self._has_point_step():
            self.apply_segments(pos, norm, x, seg, self.seed, counter, params_out=params_out, stats_out=stats_out)
        return self._finish(data, x)
