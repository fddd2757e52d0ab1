"""InferenceNet without a GPU: what it accepts, how it passes through to the wrapped model, and its MLP plan."""
import pytest
import torch

import _seeded as S


def big(use_crf):
    from crfconv_amd import models
    return models.PointConvBig(6, 13, use_crf=use_crf, steps=2)


def test_other_networks_are_refused_with_a_typeerror_that_names_what_is_accepted():
    from crfconv_amd import InferenceNet, models
    with pytest.raises(TypeError, match='PointConvBig'):
        InferenceNet(models.CRFSegNet(6, 13))
    with pytest.raises(TypeError, match='PointConvBig'):
        InferenceNet(torch.nn.Linear(4, 4))
    mixed = big(True)
    mixed.deconv2 = models.point_conv_big.Upsampling(128, 64, 64)
    with pytest.raises(TypeError, match='all CRF layers or all Upsampling'):
        InferenceNet(mixed)


@pytest.mark.parametrize('use_crf', [True, False])
def test_construction_on_a_cpu_model_and_pass_through(use_crf):
    import crfconv_amd
    net = big(use_crf)
    fast = crfconv_amd.InferenceNet(net)
    assert list(fast.children()) == [net]
    assert fast.training is True and crfconv_amd.InferenceNet(big(use_crf).eval()).training is False      # it starts in the model's mode
    # state_dict: the model's keys under one prefix, and a round trip through load_state_dict
    sd = fast.state_dict()
    assert list(sd) == ['model.' + k for k in net.state_dict()]
    other = S.fill_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, 31)
    fast.load_state_dict({'model.' + k: v for k, v in other.items()})
    for k, v in net.state_dict().items():
        assert torch.equal(v, other[k]), k
    twin = crfconv_amd.InferenceNet(big(use_crf))
    twin.load_state_dict(fast.state_dict())
    for (ka, va), (kb, vb) in zip(twin.state_dict().items(), sd.items()):
        assert ka == kb and torch.equal(va, fast.state_dict()[ka])
    # train() / eval() reach the model
    fast.eval()
    assert fast.training is False and all(m.training is False for m in net.modules())
    fast.train()
    assert fast.training is True and all(m.training is True for m in net.modules())
    fast.train(False)
    assert net.training is False


def test_a_training_mode_call_raises_before_anything_runs():
    from crfconv_amd import InferenceNet
    fast = InferenceNet(big(True))
    fast.train()
    with pytest.raises(RuntimeError, match='eval'):
        fast(object())


@pytest.mark.parametrize('use_crf,count', [(True, 50), (False, 34)])
def test_the_mlp_plan_lists_every_batchnorm_mlp_outside_weight_nn_once(use_crf, count):
    from crfconv_amd import InferenceNet
    from crfconv_amd.models.common import MLP
    net = big(use_crf)
    plan = InferenceNet(net).mlp_plan()
    names = [n for n, _ in plan]
    assert len(names) == len(set(names)) == count
    assert len({id(m) for _, m in plan}) == count
    # counted independently, by the state_dict: one entry per running_mean outside the per-edge weight MLPs
    want = sorted(k[:-len('.bn.batch_norm.running_mean')] for k in net.state_dict()
                  if k.endswith('.bn.batch_norm.running_mean') and '.weight_nn.' not in k)
    assert sorted(names) == want
    for n, m in plan:
        assert isinstance(m, MLP) and m.bn is not None and net.get_submodule(n) is m
    # 20 encoder lin_in / lin_out, 5 shortcuts, the classifier head, and 6 (CRF) or 2 (Upsampling) per decoder
    assert sum(n.endswith(('lin_in', 'lin_out')) for n in names) == 20
    assert sum(n.endswith('shortcut') for n in names) == 5
    assert sum(n.startswith('deconv') for n in names) == (24 if use_crf else 8)
    assert 'classifier.0' in names
