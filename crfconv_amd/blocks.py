"""Sliding XY blocks of scenes on the device, for ragged batches (csrc/blocks.hip).

The reference's second data route -- ``process_raw_path`` of datasets/scannet_dataset.py:58-117, s3dis_dataset.py:119-171,
semantic3d_dataset.py:107-157 and npm3d_dataset.py:90-144 -- aligns a scene to its minimum corner, lays a grid of blocks of
``block_size`` every ``stride`` metres, gives each block the points inside it plus a ``padding`` ring, and drops blocks with fewer than
``min_points`` points or with less than ``proportion`` of them inside the un-padded core.  ``sliding_blocks`` does that for all scenes
of a batch at once and returns the blocks as ONE ragged batch -- ``ptr`` / ``batch`` over rows, the form ``CRFSegNet`` and the other
sparse networks take --, bit for bit the blocks of the reference's NumPy loop and in its order:

    split = blocks.sliding_blocks(pos, ptr, **blocks.SCANNET)
    pos_b, x = split.features('room')
    data = split.as_data(x, split.take(labels))

There is one host read (the block and row totals, which size the outputs) and no Python loop over blocks or scenes.

The networks return one row of scores per block ROW; ``BlockVotes`` (csrc/block_votes.hip) brings them back to the points of the scenes --
a point lies in up to 64 blocks -- by a sum in a fixed order over the point's rows: the same bits in every run, no float atomics:

    votes = blocks.BlockVotes(split, num_classes, core='prefer', exp=True)      # exp: the networks return log_softmax
    for b0 in range(0, split.n_blocks, 32):                                     # the network over chunks of blocks
        data, row_offset = split.select(b0, min(b0 + 32, split.n_blocks), x)
        votes.update(net(data).detach(), row_offset)                            # ONE launch, no host read
    scores, pred = votes.result('mean')                                         # pred = -1 where no kept block covers the point
    hist = votes.confusion(labels)                                              # int64 [C, C]: feeds runningScore / iou_from_confusions
"""
import ctypes
import math

import torch

from . import _lib
from .data import Data

# the four parameter sets, from the reference's dataset constructors (scannet_dataset.py:33-37, s3dis_dataset.py:55-59,
# semantic3d_dataset.py:52-56, npm3d_dataset.py:32-36) and the form of their block-count lines (:82 / :136 / :117 / :102)
SCANNET = dict(block_size=1.5, stride=1.0, padding=0.2, min_points=200, proportion=0.02, count_form='ratio')
S3DIS = dict(block_size=1.0, stride=0.5, padding=0.1, min_points=100, proportion=0.02, count_form='ratio')
SEMANTIC3D = dict(block_size=5.0, stride=3.0, padding=0.5, min_points=500, proportion=0.02, count_form='ceil_first')
NPM3D = dict(block_size=5.0, stride=3.0, padding=0.5, min_points=500, proportion=0.02, count_form='ceil_first')

COUNT_FORMS = {'ratio': 0, 'ceil_first': 1}
FEATURE_FORMS = {'room': 0, 'block': 1}
MAX_MEMBERSHIPS = 64          # blocks one point may lie in: (ceil((block_size + 2 padding) / stride) + 1) ** 2
CELL_CAP = 1 << 16            # grid cells the first attempt has room for; a larger grid costs one more attempt (and host read)
_LIMIT = 1 << 31

_STATUS_BAD_PTR, _STATUS_CELL_CAP, _STATUS_OVERFLOW = 1, 2, 4
CORE_MODES = {'all': 0, 'only': 1, 'prefer': 2}
REDUCE_FORMS = {'sum': 0, 'mean': 1}
MAX_CLASSES = 64              # classes BlockVotes takes: a workgroup holds whole points


def memberships_bound(block_size, stride, padding):
    """The most blocks one point can lie in: (ceil((block_size + 2 padding) / stride) + 1) ** 2."""
    return (int(math.ceil((block_size + 2.0 * padding) / stride)) + 1) ** 2


class BlockSplit:
    """The blocks of ``sliding_blocks``, device tensors: ptr [n_blocks + 1] int64 row ranges; per row indices (scene-local point index,
    the reference's ``indices``), rows (row of ``pos``), mask int8 (in the block's un-padded core), batch (block id), all [R]; per block
    scene [n_blocks] int64 and cell [n_blocks, 2] int32 = (i, j); per scene pos_min and limit [S, 3] float32; n_blocks, n_rows ints."""

    def __init__(self, pos, ptr, indices, rows, mask, batch, scene, cell, pos_min, limit):
        self._pos = pos
        self.ptr, self.indices, self.rows, self.mask, self.batch = ptr, indices, rows, mask, batch
        self.scene, self.cell, self.pos_min, self.limit = scene, cell, pos_min, limit
        self.n_blocks, self.n_rows = scene.shape[0], rows.shape[0]
        self._pos_block = None
        self._reverse = self._rev_packed = self._ptr_host = None

    def take(self, t):
        """t[rows]: a per-point tensor (labels, colours) gathered to the rows of the blocks."""
        if t.shape[0] != self._pos.shape[0]:
            raise ValueError('BlockSplit.take: %d rows, the split was made of %d points' % (t.shape[0], self._pos.shape[0]))
        return t[self.rows]

    def features(self, form, extra=None):
        """(pos_block [R, 3], x [R, 3 + F]) from the aligned positions a = pos - pos_min[scene]; extra [N, F] float32 per point.
        form='room': x = cat(extra, a / limit) (s3dis_dataset.py:132, :161; ScanNet with extra=None, scannet_dataset.py:78, :107);
        form='block': x = cat(a - centre, extra), centre = (block_min + block_max) / 2 over the block's rows with z = block_min.z
        (semantic3d_dataset.py:142-149, npm3d_dataset.py:127-136).  pos_block = a[rows]."""
        from .graph import ptr as p_, stream_ptr
        if form not in FEATURE_FORMS:
            raise ValueError("BlockSplit.features: form must be 'room' or 'block', got %r" % (form,))
        pos, dev = self._pos, self._pos.device
        N, F = pos.shape[0], 0
        if extra is not None:
            if not (extra.is_cuda and extra.dtype == torch.float32 and extra.dim() == 2 and extra.shape[0] == N):
                raise ValueError('BlockSplit.features: extra must be a float32 device tensor [N, F]')
            extra, F = extra.contiguous(), extra.shape[1]
            if F == 0:
                extra = None
        R = self.n_rows
        pos_block = torch.empty((R, 3), dtype=torch.float32, device=dev)
        x = torch.empty((R, 3 + F), dtype=torch.float32, device=dev)
        if R:
            bounds = torch.empty((self.n_blocks, 6), dtype=torch.float32, device=dev) if form == 'block' else None
            _lib.call('crfconv_sliding_blocks_features', p_(pos), N, p_(self.pos_min), p_(self.limit), self.pos_min.shape[0], p_(extra), F,
                      p_(self.rows), p_(self.batch), p_(self.ptr), p_(self.scene), self.n_blocks, R, FEATURE_FORMS[form], p_(bounds),
                      p_(pos_block), p_(x), stream_ptr())
        self._pos_block = pos_block
        return pos_block, x

    def as_data(self, x, y=None):
        """``Data(pos, x, y, batch, ptr, mask, indices)`` of the blocks: what the reference saves per block, as one ragged batch."""
        if x.shape[0] != self.n_rows or (y is not None and y.shape[0] != self.n_rows):
            raise ValueError('BlockSplit.as_data: x and y must have one row per block row (%d)' % self.n_rows)
        pos_block = self._pos_block if self._pos_block is not None else self.features('room')[0]
        return Data(pos=pos_block, x=x, y=y, batch=self.batch, ptr=self.ptr, mask=self.mask, indices=self.indices)

    def select(self, b0, b1, x, y=None):
        """(``Data`` of blocks b0 .. b1, row_offset): pos, x, y, mask and indices sliced to the rows of those blocks, batch - b0 and ptr
        rebased to start at 0 -- one chunk of the split for the network -- and the first row of the chunk, what ``BlockVotes.update``
        takes beside the chunk's scores.  The row ranges come from a host copy of ptr, read once and kept."""
        if x.shape[0] != self.n_rows or (y is not None and y.shape[0] != self.n_rows):
            raise ValueError('BlockSplit.select: x and y must have one row per block row (%d)' % self.n_rows)
        b0, b1 = int(b0), int(b1)
        if not 0 <= b0 <= b1 <= self.n_blocks:
            raise ValueError('BlockSplit.select: blocks %d .. %d outside 0 .. %d' % (b0, b1, self.n_blocks))
        if self._ptr_host is None:
            self._ptr_host = self.ptr.tolist()             # the one host read of select, at its first call
        pos_block = self._pos_block if self._pos_block is not None else self.features('room')[0]
        r0, r1 = self._ptr_host[b0], self._ptr_host[b1]
        rows = slice(r0, r1)
        return Data(pos=pos_block[rows], x=x[rows], y=None if y is None else y[rows], batch=self.batch[rows] - b0,
                    ptr=self.ptr[b0:b1 + 1] - r0, mask=self.mask[rows], indices=self.indices[rows]), r0

    def _reverse_packed(self):
        """(rev_ptr, the list entries as the library wrote them: the row in bits 0..30, the core flag in bit 31), built once."""
        from .graph import ptr as p_, stream_ptr
        if self._rev_packed is None:
            N, R, dev = self._pos.shape[0], self.n_rows, self._pos.device
            if N == 0 or R == 0:
                self._rev_packed = (_zeros(N + 1, torch.int64, dev), torch.empty(0, dtype=torch.int32, device=dev))
            else:
                rev_ptr = torch.empty(N + 1, dtype=torch.int64, device=dev)
                packed = torch.empty(R, dtype=torch.int32, device=dev)
                nbytes = _lib.call('crfconv_block_reverse_workspace', N, R)
                ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
                _lib.call('crfconv_block_reverse', p_(self.rows), R, N, p_(self.mask), p_(ws), nbytes, p_(rev_ptr), p_(packed), stream_ptr())
                self._rev_packed = (rev_ptr, packed)
        return self._rev_packed

    def reverse(self):
        """(rev_ptr [N + 1] int64, rev_rows [R] int32): rev_rows[rev_ptr[p] : rev_ptr[p + 1]] are the block rows r with rows[r] == p,
        ascending.  Built at the first call by a stable sort (no atomics: the same bits in every run) and kept on the split."""
        if self._reverse is None:
            rev_ptr, packed = self._reverse_packed()
            self._reverse = (rev_ptr, packed & 0x7fffffff)
        return self._reverse


class BlockVotes:
    """Scores per block row summed onto the points of the split's scenes, deterministically (csrc/block_votes.hip).

    ``update(scores, row_offset)`` adds, for every point, the scores of its rows among row_offset .. row_offset + len(scores) in
    ascending row order (float32, one add per row, then one add onto ``sums``) and the number of rows to ``count``; with exp=True the
    terms are expf(score).  core: 'all' rows of a point, 'only' those in their block's un-padded core (mask == 1), 'prefer' the core rows
    of a point that has one anywhere in the split and all rows of a point that has none.  sums [N, C] float32 and count [N] int32 are
    public.  No backward."""

    def __init__(self, split, num_classes, core='prefer', exp=False):
        if not isinstance(split, BlockSplit):
            raise ValueError('BlockVotes: split must be the BlockSplit of sliding_blocks')
        if core not in CORE_MODES:
            raise ValueError("BlockVotes: core must be 'all', 'only' or 'prefer', got %r" % (core,))
        C = int(num_classes)
        if not 1 <= C <= MAX_CLASSES:
            raise ValueError('BlockVotes: num_classes = %d outside 1 .. %d' % (C, MAX_CLASSES))
        self.split, self.num_classes, self.core, self.exp = split, C, core, bool(exp)
        self._rev_ptr, self._rev_rows = split._reverse_packed()
        self.n_points, dev = split._pos.shape[0], split._pos.device
        self.sums = torch.zeros((self.n_points, C), dtype=torch.float32, device=dev)
        self.count = torch.zeros(self.n_points, dtype=torch.int32, device=dev)
        self._bad = torch.zeros(1, dtype=torch.int32, device=dev)

    def reset(self):
        self.sums.zero_()
        self.count.zero_()

    def update(self, scores, row_offset=0):
        """scores [R', C] float32 on the device: the scores of block rows row_offset .. row_offset + R' (row_offset a host int, as
        ``BlockSplit.select`` returns it).  ONE library call, no host read: capturable."""
        from .graph import ptr as p_, stream_ptr
        C, R = self.num_classes, self.split.n_rows
        if not (torch.is_tensor(scores) and scores.dim() == 2 and scores.shape[1] == C and scores.dtype == torch.float32):
            raise ValueError('BlockVotes.update: scores must be a float32 tensor [rows, %d]' % C)
        if not scores.is_cuda:
            raise ValueError('BlockVotes.update: scores must be on the device (got %s); there is no CPU path' % scores.device)
        row_offset, n = int(row_offset), scores.shape[0]
        if row_offset < 0 or row_offset + n > R:
            raise ValueError('BlockVotes.update: rows %d .. %d outside the split\'s 0 .. %d' % (row_offset, row_offset + n, R))
        if n == 0 or self.n_points == 0:
            return
        scores = scores.detach().contiguous()
        _lib.call('crfconv_block_votes_update', p_(scores), n, row_offset, C, p_(self._rev_ptr), p_(self._rev_rows), R, self.n_points,
                  CORE_MODES[self.core], 1 if self.exp else 0, p_(self.sums), p_(self.count), stream_ptr())
        for t in (self.sums, self.count):                  # written by a library kernel
            torch.autograd.graph.increment_version(t)

    def result(self, reduce='mean', fill=-1):
        """(scores_out [N, C] float32, pred [N] int64): sums ('sum') or sums / float32(count) ('mean'), and the first arg-max of sums.
        A point no row was added to has a zero row and pred = fill.  One launch, no host read."""
        from .graph import ptr as p_, stream_ptr
        if reduce not in REDUCE_FORMS:
            raise ValueError("BlockVotes.result: reduce must be 'mean' or 'sum', got %r" % (reduce,))
        N, C, dev = self.n_points, self.num_classes, self.sums.device
        out = torch.empty((N, C), dtype=torch.float32, device=dev)
        pred = torch.empty(N, dtype=torch.int64, device=dev)
        if N:
            _lib.call('crfconv_block_votes_result', p_(self.sums), p_(self.count), N, C, REDUCE_FORMS[reduce], int(fill), p_(out), p_(pred),
                      stream_ptr())
        return out, pred

    def confusion(self, labels, label_shift=0, out=None):
        """Confusion matrix of the merged votes, device int64 [C, C] (rows = ground truth), through crfconv_vote_confusion on ``sums``: the
        prediction of point p is the first arg-max of sums[p], its class labels[p] - label_shift; labels outside [0, C) are skipped, and
        so are the points no row was added to (their labels are moved outside first).  Accumulates into `out` when given."""
        from .graph import ptr as p_, require_gpu, stream_ptr
        N, C = self.n_points, self.num_classes
        if not (torch.is_tensor(labels) and labels.numel() == N):
            raise ValueError('BlockVotes.confusion: one label per point (%d) is needed' % N)
        if out is None:
            out = torch.zeros((C, C), dtype=torch.int64, device=self.sums.device)
        elif not (torch.is_tensor(out) and out.dtype == torch.int64 and tuple(out.shape) == (C, C) and out.is_contiguous()):
            raise ValueError('BlockVotes.confusion(out=): a contiguous int64 [%d, %d] tensor is needed' % (C, C))
        require_gpu(labels, out)
        if N == 0:
            return out
        labels = torch.where(self.count > 0, labels.reshape(-1).long(), int(label_shift) - 1).contiguous()
        _lib.call('crfconv_vote_confusion', p_(self.sums), N, C, None, p_(labels), N, int(label_shift), p_(out), p_(self._bad), stream_ptr())
        torch.autograd.graph.increment_version(out)
        return out


def _zeros(shape, dtype, dev):
    """Zeros on the device by a copy from the host, not a fill launch."""
    from .graph import to_device
    return to_device(torch.zeros(shape, dtype=dtype), dev)


def _empty_split(pos, S, pos_min=None, limit=None):
    """A split without blocks: empty tensors, ptr = [0]; pos_min / limit [S, 3] are zeros unless given.  No launch."""
    dev, i64 = pos.device, torch.int64
    e = lambda *shape, dtype=i64: torch.empty(shape, dtype=dtype, device=dev)            # noqa: E731
    if pos_min is None:
        pos_min, limit = _zeros((S, 3), torch.float32, dev), _zeros((S, 3), torch.float32, dev)
    return BlockSplit(pos, _zeros(1, i64, dev), e(0), e(0), e(0, dtype=torch.int8), e(0), e(0), e(0, 2, dtype=torch.int32), pos_min, limit)


def sliding_blocks(pos, ptr=None, *, block_size, stride, padding, min_points=200, proportion=0.02, count_form='ratio'):
    """The sliding blocks of the scenes of pos [N, 3] (float32, device) given by ptr [S + 1] (int64; None: one scene) -> BlockSplit.

    Per scene a = pos - min(pos) in float32 and limit = max(a); the block counts per axis come from the float32 limit in double,
    count_form='ratio': int(ceil((limit - block_size) / stride)) + 1 (ScanNet, S3DIS), 'ceil_first': int(ceil(limit - block_size) /
    stride) + 1 (Semantic3D, NPM3D -- the reference's parenthesis, kept), never below 0.  Block (i, j) begins at (i stride, j stride)
    and holds the points with f32(beg - padding) <= a <= f32((beg + block_size) + padding) on x and y; its mask is the same test without
    the padding.  A block is kept iff it has at least min_points points and mask.sum() / count >= proportion.  Kept blocks are numbered
    scene-major, then i, then j; rows inside a block ascend.  An empty scene (a repeated ptr entry) has no block and zeros for pos_min
    and limit.

    Limits: positions finite; N and the row total below 2^31; at most 2^22 blocks along x or y of a scene and fewer than 2^31 grid cells
    in the batch (ValueError otherwise); the first attempt has room for CELL_CAP = 65 536 grid cells, a batch with more is run a second
    time with the room it reported (one more host read).  Where a scene's minimum on an axis is a zero of both signs, pos_min is -0.0
    and the aligned zeros come out +0.0 (NumPy's min keeps whichever zero comes first)."""
    from .graph import ptr as p_, require_gpu, stream_ptr, to_device
    if not (torch.is_tensor(pos) and pos.dim() == 2 and pos.shape[1] == 3 and pos.dtype == torch.float32):
        raise ValueError('sliding_blocks: pos must be a float32 tensor [N, 3]')
    if not pos.is_cuda:
        raise ValueError('sliding_blocks: pos must be on the device (got %s); there is no CPU path' % pos.device)
    N, dev = pos.shape[0], pos.device
    if N >= _LIMIT:
        raise ValueError('sliding_blocks: N = %d is not below 2^31' % N)
    block_size, stride, padding, proportion = float(block_size), float(stride), float(padding), float(proportion)
    if not (stride > 0.0 and block_size > 0.0 and padding >= 0.0) or math.isinf(block_size + padding):
        raise ValueError('sliding_blocks: stride and block_size must be positive and padding non-negative')
    if count_form not in COUNT_FORMS:
        raise ValueError("sliding_blocks: count_form must be 'ratio' or 'ceil_first', got %r" % (count_form,))
    if memberships_bound(block_size, stride, padding) > MAX_MEMBERSHIPS:
        raise ValueError('sliding_blocks: a point may lie in (ceil((block_size + 2 padding) / stride) + 1)^2 = %d blocks, above %d'
                         % (memberships_bound(block_size, stride, padding), MAX_MEMBERSHIPS))
    if ptr is None:
        ptr = to_device(torch.tensor([0, N] if N else [0], dtype=torch.int64), dev)
    if not (torch.is_tensor(ptr) and ptr.dtype == torch.int64 and ptr.dim() == 1 and ptr.numel() >= 1):
        raise ValueError('sliding_blocks: ptr must be an int64 tensor [S + 1]')
    require_gpu(ptr)
    pos, ptr = pos.detach().contiguous(), ptr.contiguous()
    S = ptr.numel() - 1
    if S == 0:
        if N:
            raise ValueError('sliding_blocks: ptr names no scene but pos has %d rows' % N)
        return _empty_split(pos, 0)
    if N == 0:
        return _empty_split(pos, S)              # (every scene empty: nothing to launch)
    spec = _lib.SlidingBlocksSpec(block_size, stride, padding, proportion, int(min_points), COUNT_FORMS[count_form])
    cap = CELL_CAP
    pos_min = torch.empty((S, 3), dtype=torch.float32, device=dev)
    limit = torch.empty((S, 3), dtype=torch.float32, device=dev)
    totals = torch.empty(4, dtype=torch.int64, device=dev)
    while True:
        nbytes = _lib.call('crfconv_sliding_blocks_workspace', N, S, cap)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        _lib.call('crfconv_sliding_blocks_count', p_(pos), N, p_(ptr), S, ctypes.byref(spec), cap, p_(pos_min), p_(limit), p_(totals), p_(ws),
                  nbytes, stream_ptr())
        n_blocks, n_rows, n_cells, status = totals.tolist()                                # THE host read
        if status & _STATUS_BAD_PTR:
            raise ValueError('sliding_blocks: ptr must start at 0, end at N = %d and be non-decreasing' % N)
        if status & _STATUS_OVERFLOW:
            raise ValueError('sliding_blocks: a scene has more than 2^22 blocks along an axis, or the batch 2^31 grid cells or more')
        if not status & _STATUS_CELL_CAP:
            break
        cap = n_cells                            # (known exactly now: the second attempt is the last)
    if n_rows >= _LIMIT:
        raise ValueError('sliding_blocks: %d rows in the blocks, not below 2^31' % n_rows)
    if n_blocks == 0:
        return _empty_split(pos, S, pos_min, limit)
    i64 = torch.int64
    out_ptr = torch.empty(n_blocks + 1, dtype=i64, device=dev)
    rows, indices, batch = (torch.empty(n_rows, dtype=i64, device=dev) for _ in range(3))
    mask = torch.empty(n_rows, dtype=torch.int8, device=dev)
    scene = torch.empty(n_blocks, dtype=i64, device=dev)
    cell = torch.empty((n_blocks, 2), dtype=torch.int32, device=dev)
    ebytes = _lib.call('crfconv_sliding_blocks_emit_workspace', N, n_rows)
    ews = torch.empty(ebytes, dtype=torch.uint8, device=dev)
    _lib.call('crfconv_sliding_blocks_emit', p_(pos), N, p_(ptr), S, ctypes.byref(spec), cap, p_(pos_min), n_blocks, n_rows, p_(ws), nbytes,
              p_(ews), ebytes, p_(out_ptr), p_(rows), p_(indices), p_(mask), p_(batch), p_(scene), p_(cell), stream_ptr())
    return BlockSplit(pos, out_ptr, indices, rows, mask, batch, scene, cell, pos_min, limit)
