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
"""
import ctypes

import numpy as np
import torch

_AUG_DOMAIN = 0xA0761D6478BD642F          # csrc/augment.hip: AUG_DOMAIN
_M64 = 0xFFFFFFFFFFFFFFFF


class _Transform:
    """A lone transform applies as a Compose of one."""

    def __call__(self, data):
        if getattr(self, '_compose', None) is None:
            self._compose = Compose([self])
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


class Compose:
    """The chain, validated and lowered to one crfconv_augment call.  `generator`: the seed is ONE draw on it at construction (on
    data._private_generator() when None: the global generator never advances); a device counter advances per call.
    ``state_dict()`` / ``load_state_dict()`` carry seed and counter."""

    def __init__(self, transforms, generator=None):
        flat = []
        for t in transforms:
            flat.extend(t.transforms if isinstance(t, Compose) else [t])
        self.transforms = flat
        self.rotate = self.scale = self.symmetry = self.noise = self.drop = self.add = None
        last = -1
        for t in flat:
            k = next((i for i, cls in enumerate(_ORDER) if type(t) is cls), None)
            if k is None:
                raise NotImplementedError('Compose: %r is not supported (supported: %s)' % (t, ', '.join(c.__name__ for c in _ORDER)))
            if k <= last:
                raise NotImplementedError('Compose: %r out of order; supported is a subsequence of %s' % (t, ' -> '.join(c.__name__ for c in _ORDER)))
            last = k
            setattr(self, ('rotate', 'scale', 'symmetry', 'noise', 'drop', 'add')[k], t)
        if self.drop is not None and self.drop.feature_name != 'rgb':
            raise NotImplementedError('Compose: %r: only the rgb feature can be dropped' % (self.drop,))
        self.add_rgb = False
        if self.add is not None:
            a = self.add
            for name in a.feat_names:
                if name not in ('pos', 'rgb'):
                    raise NotImplementedError('Compose: %r: feature %r (only pos and rgb are supported)' % (a, name))
            added = [n for n, on in zip(a.feat_names, a.list_add_to_x) if on]
            if added not in (['pos'], ['pos', 'rgb']):
                raise NotImplementedError('Compose: %r: x must be [pos] or [pos, rgb], got %s' % (a, added))
            if any(d for n, d in zip(a.feat_names, a.delete_feats) if n == 'pos'):
                raise NotImplementedError('Compose: %r: pos cannot be deleted' % (a,))
            self.add_rgb = added == ['pos', 'rgb']
        if generator is None:
            from .data import _private_generator
            generator = _private_generator()
        self.seed = int(torch.randint(0, 2 ** 62, (1,), generator=generator, dtype=torch.int64, device=generator.device).item())
        self._counter = None                   # device word, made on first use
        self._counter_value = 0

    def __repr__(self):
        return 'Compose(%s)' % ', '.join(repr(t) for t in self.transforms)

    # ---- the kernel's view of the chain
    def _spec(self):
        from ._lib import AugmentSpec
        s = AugmentSpec()
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

        def ok(t, shape):
            return (t is None or (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape))
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

    def _device_counter(self, device):
        if self._counter is None or self._counter.device != device:
            value = self._counter_value if self._counter is None else int(self._counter.item())
            self._counter = torch.full((1,), value, dtype=torch.int64, device=device)
        return self._counter

    def __call__(self, data, params_out=None):
        """One crop (``Data`` with pos [k, 3] and rgb [k, 3] on the device), augmented in place and returned, as the reference's
        transforms do; with AddFeatsByKeys, data.x = [pos, rgb] [k, C] and the deleted features are gone."""
        from . import _lib
        from .graph import ptr, require_gpu, stream_ptr
        if getattr(data, 'norm', None) is not None:
            raise NotImplementedError('Compose: data.norm is not supported (the transforms would rotate it too)')
        pos = data.pos
        require_gpu(pos)
        if pos.dim() != 2 or pos.shape[-1] != 3:
            raise ValueError('Compose: data.pos must be [k, 3], got %s' % (tuple(pos.shape),))
        if pos.dtype != torch.float32 or not pos.is_contiguous():
            pos = data.pos = pos.float().contiguous()
        rgb = getattr(data, 'rgb', None)
        if self.add_rgb and rgb is None:
            raise ValueError('Compose: %r needs data.rgb' % (self.add,))
        if self.add is not None and getattr(data, 'x', None) is not None:
            raise NotImplementedError('Compose: %r onto an existing data.x is not supported' % (self.add,))
        x = None
        if self.add_rgb or (self.drop is not None and rgb is not None):
            x = torch.cat([pos, rgb.to(torch.float32)], -1).contiguous()
        elif self.add is not None:
            x = torch.empty_like(pos)
        counter = self._device_counter(pos.device)
        _lib.call('crfconv_add_i64', ptr(counter), 1, 1, stream_ptr())
        self.apply_batch(pos[None], None if x is None else x[None], self.seed, counter,
                         params_out=None if params_out is None else params_out.view(1, 8))
        if x is not None and x.shape[-1] == 6:
            data.rgb = x[:, 3:] if self.add is None else x[:, 3:].clone()      # (after DropFeature; x keeps its own copy)
        if self.add is not None:
            data.x = x if self.add_rgb else x[:, :3].contiguous()
            for name, delete in zip(self.add.feat_names, self.add.delete_feats):
                if delete and name in data.__dict__:
                    delattr(data, name)
        return data

    def state_dict(self):
        return {'seed': int(self.seed), 'counter': int(self._counter.item()) if self._counter is not None else self._counter_value}

    def load_state_dict(self, sd):
        self.seed = int(sd['seed']) & _M64
        self._counter_value = int(sd['counter'])
        if self._counter is not None:
            self._counter.fill_(self._counter_value)
