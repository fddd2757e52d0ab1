"""The self-capturing eval forward and the fused classifier head without a GPU: what constructs, what train.stats reports for a model
that never captured, when the eval capture is wanted, and that a model's private eval runner never travels with a copy of it."""
import collections
import copy
import os
import pickle

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def big(use_crf=True):
    from crfconv_amd import models
    return models.PointConvBig(6, 13, use_crf=use_crf, steps=2)


def cpu_batch(n=64):
    """A five-level MultiScaleData on the CPU (shapes only: no kernel ever sees it)."""
    from crfconv_amd import Data, MultiScaleData
    levels, m = [], n
    for lvl in range(5):
        nxt = max(m // 2, 1)
        levels.append(Data(pos=torch.zeros(2, m, 3), neighbor_idx=torch.zeros(2, m, 4, dtype=torch.long),
                           sub_idx=torch.zeros(2, nxt, 4, dtype=torch.long), up_idx=torch.zeros(2, m, 1, dtype=torch.long)))
        m = nxt
    return MultiScaleData(x=torch.zeros(2, n, 6), multiscale=levels)


@pytest.fixture
def autograph_on():
    from crfconv_amd import train
    was = train._AUTO['on']
    train.set_autograph(True)
    try:
        yield train
    finally:
        train.set_autograph(was)


@pytest.mark.parametrize('use_crf', [True, False])
def test_inference_net_with_a_fused_head_constructs_on_a_cpu_model(use_crf):
    from crfconv_amd import InferenceNet
    net = big(use_crf).eval()
    fast = InferenceNet(net, fused_head=True)
    assert fast.fused_head is True and InferenceNet(net).fused_head is False
    assert list(fast.children()) == [net] and fast.training is False
    assert list(fast.state_dict()) == ['model.' + k for k in net.state_dict()]      # the flag adds no state


def test_stats_of_a_fresh_model_are_all_zeros_with_the_documented_keys():
    from crfconv_amd import train
    st = train.stats(big())
    assert set(st) == {'train', 'eval'}
    for which in ('train', 'eval'):
        assert set(st[which]) == {'captures', 'replays', 'eager'}
        assert st[which]['captures'] == 0 and st[which]['replays'] == 0
        assert isinstance(st[which]['eager'], collections.Counter) and sum(st[which]['eager'].values()) == 0
    # the explicit runners report under their own key, zeros before their first call
    runner = train.GraphedInference(big().eval())
    assert train.stats(runner)['eval'] == {'captures': 0, 'replays': 0, 'eager': collections.Counter()}
    assert train.stats(train.GraphedModel(big()))['train'] == {'captures': 0, 'replays': 0, 'eager': collections.Counter()}


def test_the_eval_capture_is_not_wanted_for_a_cpu_batch_nor_with_grad_enabled(autograph_on):
    train = autograph_on
    batch = cpu_batch()
    with torch.no_grad():
        assert train.autograph_eval_wanted(batch) is False              # a CPU batch
        assert train.autograph_eval_wanted(object()) is False           # no batch at all
    assert torch.is_grad_enabled()
    assert train.autograph_eval_wanted(batch) is False


def test_a_cpu_eval_forward_under_no_grad_creates_no_runner(autograph_on):
    from crfconv_amd._lib import CrfConvError
    train = autograph_on
    net = big().eval()
    with torch.no_grad(), pytest.raises(CrfConvError):                  # there is no CPU path: the model's own forward refuses, as before
        net(cpu_batch())
    assert '_autograph_eval' not in net.__dict__ and '_autograph' not in net.__dict__
    assert train.stats(net)['eval'] == {'captures': 0, 'replays': 0, 'eager': collections.Counter()}


def test_copies_and_pickles_of_a_model_drop_its_eval_runner():
    net = big().eval()
    marker = object()
    object.__setattr__(net, '_autograph_eval', marker)
    object.__setattr__(net, '_autograph', marker)
    twin = copy.deepcopy(net)
    assert '_autograph_eval' not in twin.__dict__ and '_autograph' not in twin.__dict__
    assert net.__dict__['_autograph_eval'] is marker                    # the original keeps its own
    object.__setattr__(net, '_autograph_eval', 'runner')                # (something that pickles)
    object.__setattr__(net, '_autograph', 'runner')
    back = pickle.loads(pickle.dumps(net))
    assert '_autograph_eval' not in back.__dict__ and '_autograph' not in back.__dict__
    assert list(back.state_dict()) == list(net.state_dict())
    net.float()                                                         # whatever goes through _apply drops the graphs
    assert '_autograph_eval' not in net.__dict__ and '_autograph' not in net.__dict__


def test_the_header_declares_what_it_declared():
    """The eval form of the head is reached through crfconv_head_forward: no prototype and no record was added for it."""
    from abi_counts import N_FUNCTIONS, N_RECORDS
    from crfconv_amd import _lib
    with open(os.path.join(ROOT, 'include', 'crfconv_amd.h')) as f:
        text = f.read()
    functions, records = _lib.parse_header(text)
    assert len(functions) == N_FUNCTIONS and len(records) == N_RECORDS
    assert 'mask_bits == NULL' in text and 'bit-identical' in text      # the comment names the eval form and its contract


def test_only_the_stock_network_gets_a_private_eval_runner():
    """The runner replays InferenceNet's restatement of PointConvResNet._forward: a subclass with its own _forward and a model whose
    decoders InferenceNet refuses keep their own launch-by-launch forward."""
    from crfconv_amd import models, train

    class Own(models.PointConvBig):
        def _forward(self, data):
            return super()._forward(data)
    assert train._stock_network(big(True)) and train._stock_network(big(False))
    assert not train._stock_network(Own(6, 13, use_crf=True, steps=2))
    mixed = big(True)
    mixed.deconv2 = models.point_conv_big.Upsampling(128, 64, 64)
    assert not train._stock_network(mixed)
