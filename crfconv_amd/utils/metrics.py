"""``runningScore`` of the reference (utils/metrics.py:7-56) with the confusion matrix kept on the GPU.

Same constructor, ``update`` / ``get_scores`` / ``reset`` and score names; ``update`` takes the CUDA tensors the
training loop already holds (trainval.py:108 moves both to the host every step -- a device sync per step) and
``update_from_logits`` fuses the arg-max.  Only ``get_scores`` / ``confusion_matrix`` copy the n x n counts back.

``PartScores`` is the part IoU of the reference's ``runningScoreShapeNet`` for a whole ragged batch of shapes per call, with the
running state on the device (csrc/part_scores.hip, include/crfconv_parts.h); ``runningScoreShapeNet`` below scores one shape per call.
"""
import numpy as np
import torch

from .. import _lib
from ..graph import ptr, require_gpu, stream_ptr


class runningScore(object):
    def __init__(self, n_classes, ignore_index=-1, device='cuda'):
        self.n_classes = int(n_classes)
        self.ignore_index = int(ignore_index)
        self._hist = torch.zeros((self.n_classes, self.n_classes), dtype=torch.int64, device=device)
        self._bad = torch.zeros(1, dtype=torch.int32, device=device)

    def _accumulate(self, label_trues, label_preds, logits, label_shift):
        require_gpu(label_trues, label_preds, logits)
        lt = label_trues.reshape(-1).contiguous()
        if lt.dtype != torch.int64:
            lt = lt.long()
        if logits is not None:
            if logits.shape[-1] != self.n_classes:
                raise ValueError('logits have %d classes, expected %d' % (logits.shape[-1], self.n_classes))
            logits = logits.reshape(-1, self.n_classes).float().contiguous()
            n = logits.shape[0]
        else:
            label_preds = label_preds.reshape(-1).contiguous()
            if label_preds.dtype != torch.int64:
                label_preds = label_preds.long()
            n = label_preds.numel()
        if n != lt.numel():
            raise ValueError('%d labels for %d predictions' % (lt.numel(), n))
        _lib.call('crfconv_confusion_accumulate', ptr(lt), ptr(label_preds), ptr(logits), n, self.n_classes,
                  self.ignore_index, int(label_shift), ptr(self._hist), ptr(self._bad), stream_ptr())

    def update(self, label_trues, label_preds):
        """metrics.py:21-26: rows of a 2-D input are accumulated one by one there, which equals the flat histogram."""
        self._accumulate(label_trues, label_preds, None, 0)

    def update_from_logits(self, label_trues, logits, label_shift=0):
        """``update(y, logits.max(dim=1)[1])`` (trainval.py:108) in one pass; ``label_shift=1`` folds the loop's
        ``data.y.reshape(-1) - 1`` (:100)."""
        self._accumulate(label_trues, None, logits, label_shift)

    @property
    def confusion_matrix(self):
        if int(self._bad.item()):
            raise ValueError('%d predictions outside [0, %d)' % (int(self._bad.item()), self.n_classes))
        return self._hist.cpu().numpy().astype(np.float64)

    def get_scores(self):
        """The four scores and the per-class IoU table of metrics.py:28-56, from the host copy of the counts (one
        sync).  Rows = ground truth, columns = prediction; classes with an empty row / union give nan and drop out
        of the nan-means, exactly as there."""
        cm = self.confusion_matrix
        hit = np.diag(cm)
        n_true, n_pred, total = cm.sum(axis=1), cm.sum(axis=0), cm.sum()
        with np.errstate(divide='ignore', invalid='ignore'):
            iou = hit / (n_true + n_pred - hit)
            share = n_true / total
            scores = {
                'Overall Acc': hit.sum() / total,
                'Mean Acc': np.nanmean(hit / n_true),
                'FreqW Acc': (share[share > 0] * iou[share > 0]).sum(),
                'Mean IoU': np.nanmean(iou),
            }
        return scores, {c: iou[c] for c in range(self.n_classes)}

    def reset(self):
        self._hist.zero_()
        self._bad.zero_()


class runningScoreShapeNet(object):
    """Per-shape part IoU of the reference (utils/metrics.py:59-119): ``update(label_trues, label_preds, category)``
    scores ONE shape -- the mean over the parts of its object category of |true & pred| / |true | pred|, both counts
    offset by float32 eps as there -- and ``get_scores()`` returns (instance mIoU, category mIoU, per-category table).
    The per-part intersections / unions come from the device confusion kernel (one 50 x 50 histogram per shape)."""

    obj_classes = {'Airplane': 0, 'Bag': 1, 'Cap': 2, 'Car': 3, 'Chair': 4, 'Earphone': 5, 'Guitar': 6, 'Knife': 7,
                   'Lamp': 8, 'Laptop': 9, 'Motorbike': 10, 'Mug': 11, 'Pistol': 12, 'Rocket': 13, 'Skateboard': 14,
                   'Table': 15}
    seg_classes = {'Earphone': [16, 17, 18], 'Motorbike': [30, 31, 32, 33, 34, 35], 'Rocket': [41, 42, 43],
                   'Car': [8, 9, 10, 11], 'Laptop': [28, 29], 'Cap': [6, 7], 'Skateboard': [44, 45, 46],
                   'Mug': [36, 37], 'Guitar': [19, 20, 21], 'Bag': [4, 5], 'Lamp': [24, 25, 26, 27],
                   'Table': [47, 48, 49], 'Airplane': [0, 1, 2, 3], 'Pistol': [38, 39, 40],
                   'Chair': [12, 13, 14, 15], 'Knife': [22, 23]}
    N_PARTS = 50

    def __init__(self, device='cuda'):
        self._names = {v: k for k, v in self.obj_classes.items()}
        self._score = runningScore(self.N_PARTS, ignore_index=-1, device=device)
        self.category_IoU = np.zeros(16, dtype=np.float32)
        self.category_num = np.zeros(16, dtype=np.int32)

    def update(self, label_trues, label_preds, category):
        parts = self.seg_classes[self._names[int(category)]]
        self._score.reset()
        self._score.update(label_trues, label_preds)
        cm = self._score.confusion_matrix
        eps = np.finfo(np.float32).eps
        iu = 0.0
        for l in parts:
            inter = cm[l, l]
            union = cm[l, :].sum() + cm[:, l].sum() - inter
            iu += (inter + eps) / (union + eps)
        iu /= len(parts)
        self.category_IoU[int(category)] += iu
        self.category_num[int(category)] += 1
        return iu

    def get_scores(self):
        with np.errstate(divide='ignore', invalid='ignore'):
            per_class = self.category_IoU / self.category_num
            pIoU = self.category_IoU.sum() / self.category_num.sum()
        return pIoU, per_class.mean(), {k: per_class[v] for k, v in self.obj_classes.items()}


class PartScores(object):
    """Part IoU of ragged batches of shapes on the device: what the reference's ``runningScoreShapeNet`` (utils/metrics.py:58-112) computes
    when its ``update`` is called shape by shape in batch order, bit for bit, in one library call per batch and without a host read.

        ps = PartScores.shapenet(device='cuda')      # or PartScores(parts=[[0, 1, 2, 3], [4, 5], ..], names=[..], n_labels=50)
        iou = ps.update(y, ptr, category, scores=out)                  # float64 [S], a device tensor of its own
        pIoU, mpIoU, table = ps.get_scores()                           # the one host read

    ``parts[c]`` lists the part labels of object category c: distinct, ascending, inside [0, n_labels), at least one; at most 64
    categories and 64 labels.  Shape s of a batch owns rows ptr[s] .. ptr[s + 1] and has the category ``category[s]``.  With ``scores``
    [N, n_labels] (logits, log-probabilities or summed votes) the prediction of a row is the first arg-max over the parts of its shape's
    category (``restrict=True``, the usual ShapeNet protocol) or over all columns (``restrict=False``); ties go to the lowest label.

    The per-shape value is the mean over the category's parts of (I + eps) / (U + eps) in float64, eps = float32 machine epsilon, and it
    is added onto the float32 ``category_IoU[c]`` with one rounding per shape, in batch order: NumPy's ``category_IoU[c] += iu``.

    A shape whose category is outside the table or whose bounds are not 0 <= ptr[s] <= ptr[s + 1] <= N gets NaN, is left out of the
    state and is counted; ``get_scores`` / ``category_IoU`` / ``category_num`` then raise ValueError naming the count (``reset`` clears
    it).  ``update`` and ``predict`` check their arguments on the host only as far as that needs no read of device memory.

    ``scores`` must be float32 [N, n_labels]; a view that is not contiguous is taken as its contiguous copy (one framework copy), every
    other dtype is refused rather than converted."""

    SHAPENET_NAMES = ('Airplane', 'Bag', 'Cap', 'Car', 'Chair', 'Earphone', 'Guitar', 'Knife', 'Lamp', 'Laptop', 'Motorbike', 'Mug',
                      'Pistol', 'Rocket', 'Skateboard', 'Table')
    MAX_LABELS = MAX_CATEGORIES = 64

    def __init__(self, parts, names=None, n_labels=None, device='cuda'):
        try:
            parts = [[int(l) for l in lst] for lst in parts]
        except (TypeError, ValueError):
            raise ValueError('PartScores: parts must be a list of lists of integer part labels')
        if not 1 <= len(parts) <= self.MAX_CATEGORIES:
            raise ValueError('PartScores: %d categories, expected 1..%d' % (len(parts), self.MAX_CATEGORIES))
        if n_labels is None:
            n_labels = 1 + max((l for lst in parts for l in lst), default=0)
        n_labels = int(n_labels)
        if not 1 <= n_labels <= self.MAX_LABELS:
            raise ValueError('PartScores: n_labels = %d outside 1..%d' % (n_labels, self.MAX_LABELS))
        for c, lst in enumerate(parts):
            if not lst:
                raise ValueError('PartScores: the part list of category %d is empty' % c)
            if any(b <= a for a, b in zip(lst, lst[1:])):
                raise ValueError('PartScores: the part list of category %d is not ascending and distinct: %r' % (c, lst))
            if lst[0] < 0 or lst[-1] >= n_labels:
                raise ValueError('PartScores: the part list of category %d has a label outside [0, %d): %r' % (c, n_labels, lst))
        names = ['%d' % c for c in range(len(parts))] if names is None else [str(n) for n in names]
        if len(names) != len(parts) or len(set(names)) != len(names):
            raise ValueError('PartScores: names must be %d distinct category names' % len(parts))
        self.parts, self.names, self.n_labels, self.n_cat = parts, names, n_labels, len(parts)
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise ValueError('PartScores: the state lives on the device (got %s); there is no CPU path' % self.device)
        self._state = None                                 # (parts_ptr, parts, cat_sum, cat_num, bad): made at the first use
        self._workspace = None

    @classmethod
    def shapenet(cls, device='cuda'):
        """The ShapeNet part table of the reference: 16 object categories over 50 part labels."""
        ref = runningScoreShapeNet
        names = sorted(ref.obj_classes, key=ref.obj_classes.get)
        return cls([ref.seg_classes[n] for n in names], names=names, n_labels=ref.N_PARTS, device=device)

    # ------------------------------------------------------------------------------------------------------------------- device state
    def _tensors(self):
        if self._state is None:
            from ..graph import to_device
            bounds = np.concatenate([[0], np.cumsum([len(lst) for lst in self.parts])]).astype(np.int32)
            flat = np.concatenate([np.asarray(lst, dtype=np.int32) for lst in self.parts])
            dev = self.device
            self._state = (to_device(torch.from_numpy(bounds), dev), to_device(torch.from_numpy(flat), dev),
                           torch.zeros(self.n_cat, dtype=torch.float32, device=dev), torch.zeros(self.n_cat, dtype=torch.int32, device=dev),
                           torch.zeros(1, dtype=torch.int32, device=dev))
        return self._state

    def _batch(self, what, N, ptr, category, tensors):
        """The checks that ``update`` and ``predict`` share; returns (ptr, category, S), contiguous."""
        if not (torch.is_tensor(ptr) and ptr.dtype == torch.int64 and ptr.dim() == 1 and ptr.numel() >= 1):
            raise ValueError('PartScores.%s: ptr must be an int64 tensor [S + 1]' % what)
        S = ptr.numel() - 1
        if not (torch.is_tensor(category) and category.dtype == torch.int64 and tuple(category.shape) == (S,)):
            raise ValueError('PartScores.%s: category must be an int64 tensor [S] with S = %d' % (what, S))
        if N >= 1 << 31:
            raise ValueError('PartScores.%s: N = %d is not below 2^31' % (what, N))
        if S == 0 and N:
            raise ValueError('PartScores.%s: ptr names no shape but there are %d rows' % (what, N))
        for name, t in tensors + (('ptr', ptr), ('category', category)):
            if t is not None and (t.device.type != 'cuda' or self.device.index not in (None, t.device.index)):
                raise ValueError('PartScores.%s: %s must be on the device %s (got %s); there is no CPU path' % (what, name, self.device, t.device))
        return ptr.contiguous(), category.contiguous(), S

    def _scores(self, what, scores):
        if not (torch.is_tensor(scores) and scores.dtype == torch.float32 and scores.dim() == 2):
            raise ValueError('PartScores.%s: scores must be a float32 tensor [N, %d]' % (what, self.n_labels))
        if scores.shape[1] != self.n_labels:
            raise ValueError('PartScores.%s: scores have %d columns, the part table has %d labels' % (what, scores.shape[1], self.n_labels))

    # ------------------------------------------------------------------------------------------------------------------------- entries
    def update(self, label_trues, ptr, category, scores=None, preds=None, restrict=True, return_counts=False, return_preds=False):
        """One batch of S shapes -> their part IoU, float64 [S] on the device (NaN for a bad shape); the running state takes them in.
        label_trues [N] int64; exactly one of scores [N, n_labels] float32 and preds [N] int64; ptr [S + 1] int64; category [S] int64.
        ``return_counts``: also counts int32 [S, 3, n_labels], the rows I, T, P per label (zero outside the shape's list);
        ``return_preds``: also the predictions int64 [N].  Extras follow the IoU in that order.  Nothing is read back."""
        from ..graph import ptr as p_, stream_ptr
        if (scores is None) == (preds is None):
            raise ValueError('PartScores.update: exactly one of scores and preds must be given')
        if not (torch.is_tensor(label_trues) and label_trues.dtype == torch.int64 and label_trues.dim() == 1):
            raise ValueError('PartScores.update: label_trues must be an int64 tensor [N]')
        N = label_trues.numel()
        if scores is not None:
            self._scores('update', scores)
            if scores.shape[0] != N:
                raise ValueError('PartScores.update: %d rows of scores for %d labels' % (scores.shape[0], N))
        elif not (torch.is_tensor(preds) and preds.dtype == torch.int64 and tuple(preds.shape) == (N,)):
            raise ValueError('PartScores.update: preds must be an int64 tensor [N] with N = %d' % N)
        ptr, category, S = self._batch('update', N, ptr, category, (('label_trues', label_trues), ('scores', scores), ('preds', preds)))
        dev, C = self.device, self.n_labels
        iou = torch.empty(S, dtype=torch.float64, device=dev)
        counts = torch.empty((S, 3, C), dtype=torch.int32, device=dev) if return_counts else None
        pred_out = torch.empty(N, dtype=torch.int64, device=dev) if return_preds else None
        if S:
            parts_ptr, parts, cat_sum, cat_num, bad = self._tensors()
            nbytes = 0
            if counts is None:                             # (counts_out holds the counters itself when it is asked for)
                nbytes = _lib.call('crfconv_part_scores_workspace', S, C)
                if self._workspace is None or self._workspace.numel() < nbytes:
                    self._workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            label_trues = label_trues.contiguous()
            scores = None if scores is None else scores.detach().contiguous()
            preds = None if preds is None else preds.contiguous()
            _lib.call('crfconv_part_scores_update', p_(label_trues), p_(preds), p_(scores), N, C, p_(ptr), p_(category), S, p_(parts_ptr),
                      p_(parts), self.n_cat, int(bool(restrict)), p_(self._workspace) if nbytes else None, nbytes, p_(pred_out), p_(iou),
                      p_(counts), p_(cat_sum), p_(cat_num), p_(bad), stream_ptr())
        out = (iou,) + ((counts,) if return_counts else ()) + ((pred_out,) if return_preds else ())
        return out[0] if len(out) == 1 else out

    def predict(self, scores, ptr, category, restrict=True):
        """The predictions int64 [N] of scores [N, n_labels] float32 alone, as ``update`` forms them; -1 for a row of no shape and, with
        ``restrict``, for the rows of a shape whose category is outside the table.  Nothing is read back."""
        from ..graph import ptr as p_, stream_ptr
        self._scores('predict', scores)
        N = scores.shape[0]
        ptr, category, S = self._batch('predict', N, ptr, category, (('scores', scores),))
        pred = torch.empty(N, dtype=torch.int64, device=self.device)
        if S:
            parts_ptr, parts = self._tensors()[:2]
            scores = scores.detach().contiguous()
            _lib.call('crfconv_part_predict', p_(scores), N, self.n_labels, p_(ptr), p_(category), S, p_(parts_ptr), p_(parts), self.n_cat,
                      int(bool(restrict)), p_(pred), stream_ptr())
        return pred

    # ---------------------------------------------------------------------------------------------------------------- the host's side
    def _host(self):
        """(category_IoU float32 [n_cat], category_num int32 [n_cat]): THE host read."""
        if self._state is None:
            return np.zeros(self.n_cat, dtype=np.float32), np.zeros(self.n_cat, dtype=np.int32)
        _, _, cat_sum, cat_num, bad = self._state
        n_bad = int(bad.item())
        if n_bad:
            raise ValueError('PartScores: %d shapes had a category outside [0, %d) or bounds outside their batch; reset() clears the state'
                             % (n_bad, self.n_cat))
        return cat_sum.cpu().numpy(), cat_num.cpu().numpy()

    @property
    def category_IoU(self):
        return self._host()[0]

    @property
    def category_num(self):
        return self._host()[1]

    def get_scores(self):
        """(instance mIoU, category mIoU, {category name: its mean IoU}): the reference's three values (utils/metrics.py:105-112) by the
        same NumPy expressions on the host copies; a category without a shape gives NaN there, and so does the category mIoU then."""
        category_IoU, category_num = self._host()
        with np.errstate(divide='ignore', invalid='ignore'):
            per_class = category_IoU / category_num
            pIoU = category_IoU.sum() / category_num.sum()
        return pIoU, per_class.mean(), {name: per_class[c] for c, name in enumerate(self.names)}

    def reset(self):
        if self._state is not None:
            for t in self._state[2:]:
                t.zero_()


def iou_from_confusions(confusions, eps=1e-6):
    """Trainer._iou_from_confusions (trainval.py:76-90): per-class IoU from [..., n, n] confusion counts, where a
    class that never occurs in the ground truth (row sum < 1e-3) is given the mean IoU of the classes that do."""
    cm = np.asarray(confusions, dtype=np.float64)
    hit = np.diagonal(cm, axis1=-2, axis2=-1)
    n_true, n_pred = cm.sum(axis=-1), cm.sum(axis=-2)
    iou = hit / (n_pred + n_true - hit + eps)
    absent = n_true < 1e-3
    present = (~absent).sum(axis=-1, keepdims=True)
    mean_present = iou.sum(axis=-1, keepdims=True) / (present + eps)
    return iou + absent * mean_present
