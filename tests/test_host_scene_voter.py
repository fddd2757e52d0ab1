"""No GPU: registration of the batched vote entries (crfconv_vote_update_batch, crfconv_vote_confusion), the numpy restatement of
VoteAccumulator.scores against hand-written confusion matrices, and the argument errors of update_batch / confusion / SceneVoter that are
raised before any device call."""
import os
import re
import types

import numpy as np
import pytest
import torch

from crfconv_amd import _lib
from crfconv_amd.sampling import SceneVoter, VoteAccumulator
from crfconv_amd.utils.metrics import iou_from_confusions
from s3dis_restatement import vote_repeated

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def confusion_restated(table, labels, proj_idx=None, label_shift=0):
    """crfconv_vote_confusion in numpy: first arg-max of the vote rows (through proj_idx), labels outside [0, C) skipped."""
    C = table.shape[1]
    pred = np.argmax(table if proj_idx is None else table[proj_idx], axis=1)
    true = np.asarray(labels, np.int64) - label_shift
    keep = (true >= 0) & (true < C)
    hist = np.zeros((C, C), np.int64)
    np.add.at(hist, (true[keep], pred[keep]), 1)
    return hist


def scores_restated(tables, labels, proj=None, class_proportions=None, label_shift=0):
    """VoteAccumulator.scores in numpy (trainval.py:272-287 / :304-317)."""
    conf = sum(confusion_restated(tb, labels[c], None if proj is None else proj[c], label_shift) for c, tb in enumerate(tables))
    if class_proportions is not None:
        conf = conf.astype(np.float32)
        conf *= np.expand_dims(class_proportions / (np.sum(conf, axis=1) + 1e-6), 1)
    ious = iou_from_confusions(conf)
    return float(np.mean(ious)), ious


def test_entry_points_are_registered_and_declared():
    header = open(os.path.join(ROOT, 'include', 'crfconv_amd.h')).read()
    assert 'crf_vote_desc' in header
    for name in ('crfconv_vote_update_batch', 'crfconv_vote_confusion'):
        assert name in _lib.SIGNATURES
        decl = re.search(r'int %s\((.*?)\);' % name, header, re.S)
        assert decl is not None, name
        assert len(decl.group(1).split(',')) == len(_lib.SIGNATURES[name][1]), name      # one ctypes argument per parameter
    source = open(os.path.join(ROOT, 'crfconv_amd', 'csrc', 'evaluate.hip')).read()
    assert 'crfconv_vote_update_batch' in source and 'crfconv_vote_confusion' in source
    assert 'evaluate.hip' in open(os.path.join(ROOT, 'crfconv_amd', 'csrc', 'Makefile')).read()
    fields = re.search(r'typedef struct crf_vote_desc \{(.*?)\} crf_vote_desc;', header, re.S).group(1)
    assert [f.split()[-1].rstrip(';') for f in re.sub(r'/\*.*?\*/', '', fields).strip().split('\n')] == ['test_probs', 'visits', 'last_row', 'n']


def test_scores_restatement_against_hand_written_confusions():
    """Two clouds, three classes, votes written through vote_repeated (smooth = 0: the table holds the last vote of every point); the
    confusion matrices are counted by hand."""
    C = 3
    tables = [np.zeros((5, C), np.float32), np.zeros((4, C), np.float32)]
    onehot = np.eye(C, dtype=np.float32)
    # cloud 0: points 0..4 voted classes 0, 1, 1, 2 and (point 4, named twice: the LAST row is stored) 2 then 0
    vote_repeated(tables[0], None, np.array([0, 1, 2, 3, 4, 4]), onehot[[0, 1, 1, 2, 2, 0]], 0.0)
    # cloud 1: point 0 -> class 2, point 1 -> a tie of classes 1 and 2 (the first wins), points 2, 3 unvoted (class 0)
    vote_repeated(tables[1], None, np.array([0, 1]), np.array([[0, 0, 1], [0, .5, .5]], np.float32), 0.0)
    labels = [np.array([0, 1, 2, 2, 0]), np.array([2, 1, -1, 3])]      # -1 and 3: outside [0, C), skipped
    by_hand = [np.array([[2, 0, 0], [0, 1, 0], [0, 1, 1]]), np.array([[0, 0, 0], [0, 1, 0], [0, 0, 1]])]
    for c in range(2):
        assert np.array_equal(confusion_restated(tables[c], labels[c]), by_hand[c]), c
    total = by_hand[0] + by_hand[1]                                    # [[2, 0, 0], [0, 2, 0], [0, 1, 2]]
    miou, ious = scores_restated(tables, labels)
    # IoU = hit / (row + column - hit): 2 / 2, 2 / 3, 2 / 3
    assert np.allclose(ious, [1.0, 2 / 3, 2 / 3], atol=1e-6) and abs(miou - np.mean([1.0, 2 / 3, 2 / 3])) < 1e-6
    assert np.array_equal(ious, iou_from_confusions(total))
    # through a projection: cloud 0's points seen 2, 1, 1, 3, 1 times, labels of the full cloud
    proj = [np.array([0, 0, 1, 2, 3, 3, 3, 4]), np.array([1, 0])]
    full = [np.array([0, 1, 1, 1, 2, 2, 0, 5]), np.array([1, 2])]
    hand_proj = np.array([[1, 0, 1], [1, 2, 0], [0, 0, 2]]) + np.array([[0, 0, 0], [0, 1, 0], [0, 0, 1]])
    got = sum(confusion_restated(tables[c], full[c], proj[c]) for c in range(2))
    assert np.array_equal(got, hand_proj)
    # label_shift: raw labels 1 .. C with 0 = unlabeled
    assert np.array_equal(confusion_restated(tables[0], labels[0] + 1, label_shift=1), by_hand[0])
    # class proportions (trainval.py:283): every row is rescaled to the stated number of points of its class
    prop = np.array([10, 20, 30], np.float32)
    conf = total.astype(np.float32) * (prop / (total.sum(1) + 1e-6))[:, None]
    assert np.allclose(conf.sum(1), prop, rtol=1e-5)                   # (the 1e-6 of the denominator: 5e-7 of a row of two points)
    miou_p, ious_p = scores_restated(tables, labels, class_proportions=prop)
    # rows scaled to [[10, 0, 0], [0, 20, 0], [0, 10, 20]]: IoU = 10 / 10, 20 / 30, 20 / 30
    assert np.allclose(ious_p, [1.0, 2 / 3, 2 / 3], atol=1e-6)
    prop2 = np.array([10, 20, 60], np.float32)                         # rows [[10, 0, 0], [0, 20, 0], [0, 20, 40]]: 1, 20 / 40, 40 / 60
    assert np.allclose(scores_restated(tables, labels, class_proportions=prop2)[1], [1.0, 0.5, 2 / 3], atol=1e-6)
    assert abs(miou_p - np.mean(ious_p)) < 1e-12


def test_argument_errors_are_raised_before_any_device_call():
    votes = VoteAccumulator([10, 20], 4, device='cpu')
    idx = torch.zeros((2, 8), dtype=torch.int64)
    probs = torch.zeros((2, 8, 4))
    cloud = torch.zeros((2, 1), dtype=torch.int64)
    with pytest.raises(TypeError, match='device tensor'):
        votes.update_batch(idx, [0, 1], probs=probs)
    with pytest.raises(ValueError, match='exactly one'):
        votes.update_batch(idx, cloud)
    with pytest.raises(ValueError, match='exactly one'):
        votes.update_batch(idx, cloud, probs=probs, logits=probs)
    with pytest.raises(ValueError, match='cloud_idx'):
        votes.update_batch(idx, cloud.int(), probs=probs)
    with pytest.raises(ValueError, match='cloud_idx'):
        votes.update_batch(idx, torch.zeros(3, dtype=torch.int64), probs=probs)
    with pytest.raises(ValueError, match='point_idx'):
        votes.update_batch(idx.reshape(-1), cloud, probs=probs)
    with pytest.raises(ValueError, match='holds'):
        votes.update_batch(idx, cloud, probs=probs[:, :, :3])
    with pytest.raises(_lib.CrfConvError, match='allow_repeats'):
        votes.update_batch(idx, cloud, probs=probs, repeated=True)
    with pytest.raises(_lib.CrfConvError, match='no CPU path'):       # host tensors never reach the library
        votes.update_batch(idx, cloud, probs=probs)
    with pytest.raises(ValueError, match='labels'):
        votes.confusion(0, torch.zeros(9, dtype=torch.int64))
    with pytest.raises(ValueError, match='projection'):
        votes.confusion(0, torch.zeros(9, dtype=torch.int64), proj_idx=torch.zeros(8, dtype=torch.int64))
    with pytest.raises(ValueError, match='out='):
        votes.confusion(0, torch.zeros(10, dtype=torch.int64), out=torch.zeros((4, 4), dtype=torch.int32))
    with pytest.raises(ValueError, match='per cloud'):
        votes.scores([torch.zeros(10, dtype=torch.int64)])
    assert votes._table is None

    sampler = types.SimpleNamespace(form='s3dis', rgb=[None], num_points=8, device='cpu')
    net = torch.nn.Linear(2, 2)
    with pytest.raises(ValueError, match='batch_size'):
        SceneVoter(sampler, net, votes, 0)
    with pytest.raises(ValueError, match='kernel sizes'):
        SceneVoter(sampler, net, votes, 2, kernel_size=(16, 16), ratio=(4,))
    with pytest.raises(_lib.CrfConvError, match='allow_repeats'):
        SceneVoter(sampler, net, votes, 2)
    sampler.form = 'semantic3d'
    sampler.rgb = None
    with pytest.raises(ValueError, match='colours'):
        SceneVoter(sampler, net, votes, 2)
    sampler.rgb = [None]
    voter = SceneVoter(sampler, net, votes, 2)
    with pytest.raises(ValueError, match='n_batches'):
        voter.run()
    with pytest.raises(ValueError, match='check_every'):
        voter.run(n_batches=1, check_every=0)
    assert net.training and voter.batches == 0
