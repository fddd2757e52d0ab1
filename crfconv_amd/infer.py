"""InferenceNet: the eval-mode forward of PointConvBig with every MLP block as one launch.

What ``val_one_epoch`` and ``test()`` of the reference drive (trainval.py:110-124, :170-178, :242-244) is ``model.eval()`` under
``no_grad``.  There every ``MLP`` outside a PointConv's ``weight_nn`` is a product, a coefficient launch and a BatchNorm + LeakyReLU
pass over [M, Co]; the tail of a ResNet block adds the residual join, a CRF layer's fusion a materialised ``torch.cat``.  The wrapper
runs the same forward with the product kernels' BatchNorm epilogue (``ops.linear_bn_act``): one launch per block, the coefficients of
all blocks from ONE launch at the start of the forward (``ops.bn_eval_coefs``).  Same kernels, same summation order, the same
float32 operations in the same order behind the accumulator: the logits are bit-identical to ``model.eval()(data)``.

``InferenceNet(model, fused_head=True)`` also runs the classifier -- MLP 32 -> 128, Dropout, Linear 128 -> classes -- as one launch that
never stores the [M, 128] activation (``ops.head_eval``); those logits are held to the float64 oracle's bound, not to bit-identity.

Opt-in: ``model = InferenceNet(model)`` after ``model.eval()``; what ``model.eval()(data)`` computes is untouched (under ``no_grad`` the
model replays this wrapper's default form by itself: train.GraphedInference).  Nothing is cached
across calls -- weights and running statistics are read where they live, at every call and at every replay of a captured graph."""
import torch
import torch.nn as nn

from . import _lib, ops
from .graph import table_of
from .models.common import MLP
from .models.continuous_crf_conv_big import ContinuousGaussianCRFConv as CRFConv
from .models.point_conv_big import WIDTHS, PointConvResNet, ResNetBBlock, Upsampling

JOIN_SLOPE = 0.01          # F.leaky_relu's default slope behind lin_out + shortcut (models/point_conv_big.py:84-88)


def _decoders(model):
    return [getattr(model, 'deconv%d' % (lvl + 1)) for lvl in range(len(WIDTHS) - 2, -1, -1)]


def mlp_plan(model):
    """[(qualified name, MLP)]: every BatchNorm-carrying MLP of `model` outside a PointConv's weight_nn (whose per-edge MLP lives
    inside the PointConv kernels), in module order, each once."""
    return [(name, m) for name, m in model.named_modules()
            if isinstance(m, MLP) and m.bn is not None and 'weight_nn' not in name.split('.')]


def _fused_form(mlp):
    """True where the one-launch form takes `mlp`: Linear without bias, affine BatchNorm with running statistics, no activation or a
    LeakyReLU, a channel count that is a multiple of 4.  Anything else runs the module's own eval forward."""
    bn = mlp.bn.batch_norm
    return (mlp.lin.bias is None and bn.affine and bn.running_mean is not None and bn.running_var is not None
            and (mlp.activation is None or isinstance(mlp.activation, nn.LeakyReLU)) and mlp.lin.out_features % 4 == 0)


def why_not(model):
    """None where InferenceNet takes `model`, else the TypeError's text: a PointConvBig whose decoders are all CRF layers or all
    Upsampling stages."""
    accepted = 'InferenceNet takes a PointConvBig (models.point_conv_big.PointConvResNet) whose decoders are all CRF layers or all Upsampling stages'
    if not isinstance(model, PointConvResNet):
        return '%s; got %s' % (accepted, type(model).__name__)
    kinds = {type(d) for d in _decoders(model)}
    if kinds != {CRFConv} and kinds != {Upsampling}:
        return '%s; got decoders %s' % (accepted, sorted(k.__name__ for k in kinds))
    return None


class InferenceNet(nn.Module):
    """``InferenceNet(model)(data)`` = ``model.eval()(data)`` under ``no_grad``, bit for bit, with one launch per MLP block.

    `model`: a ``PointConvBig`` (``PointConvResNet``) with CRF or ``Upsampling`` decoders; it is the wrapper's only child, so
    ``eval()`` / ``train()`` / ``to()`` / ``state_dict()`` pass through (keys under the prefix ``model.``).  Calling it in training
    mode raises.  A model with module hooks runs ``model(data)`` itself, so that the hooks fire.  Works as the ``net`` of
    ``sampling.SceneVoter`` and ``sampling.vote_scene`` and inside a caller's ``torch.cuda.graph``."""

    def __init__(self, model, fused_head=False):
        """fused_head: the classifier (MLP 32 -> 128, Dropout, Linear 128 -> classes) as ONE launch that keeps the 128 channels in
        registers (``ops.head_eval``) where the head kernel takes its shape -- at most 16 classes; anything else runs the two
        launches of the default.  Its logits may differ from the default's in the last bits (another summation order than the
        product kernels'): the contract is the logits bound against the float64 oracle, not bit-identity with ``model.eval()``."""
        super().__init__()
        self.fused_head = bool(fused_head)
        refusal = why_not(model)
        if refusal is not None:
            raise TypeError(refusal)
        self.model = model
        self.training = model.training                     # wrapped behind model.eval(): the wrapper starts in the model's mode
        self._coef_buf = {}                                # device -> the flat coefficient buffer, allocated once

    def mlp_plan(self):
        """[(name, MLP)] of the blocks the forward runs through ``ops.linear_bn_act`` where the fused form takes them."""
        return mlp_plan(self.model)

    # ------------------------------------------------------------------------------------------------------------------ forward
    def forward(self, data):
        model = self.model
        if self.training or model.training:
            raise RuntimeError('InferenceNet is the eval-mode forward: call .eval() first (training runs the model itself)')
        from . import train
        if train._has_hooks(model):
            return model(data)                             # the module calls are what fires hooks
        if data.x.dtype != torch.float32:
            raise _lib.CrfConvError('InferenceNet: float32 features only (got %s): the path computes in the reference\'s arithmetic' % data.x.dtype)
        with torch.no_grad():
            return self._forward(data)

    def _coefs(self, device):
        """{id(MLP): its [4, C] coefficient block} for the blocks of the fused form: one launch into the device's buffer."""
        mlps = [m for _, m in mlp_plan(self.model) if _fused_form(m)]
        if not mlps:
            return {}
        need = 4 * sum(m.lin.out_features for m in mlps)
        buf = self._coef_buf.get(device)
        if buf is None or buf.numel() < need:
            buf = self._coef_buf[device] = torch.empty(need, dtype=torch.float32, device=device)
        _, views = ops.bn_eval_coefs([m.bn.batch_norm for m in mlps], out=buf)
        return {id(m): v for m, v in zip(mlps, views)}

    def _mlp(self, coefs, mlp, x, skip=None, xb=None):
        """mlp([x | xb]), or leaky_relu(mlp(x) + skip, 0.01) with a skip: one launch where the fused form applies."""
        coef = coefs.get(id(mlp)) if isinstance(mlp, MLP) else None
        if coef is not None and (skip is None or mlp.activation is None):
            if skip is not None:
                return ops.linear_bn_act(x, mlp.lin.weight, coef, slope=JOIN_SLOPE, skip=skip)
            slope = 1.0 if mlp.activation is None else mlp.activation.negative_slope
            return ops.linear_bn_act(x, mlp.lin.weight, coef, slope=slope, xb=xb)
        if xb is not None:
            x = ops.cat2(x, xb)
        y = mlp(x)
        return y if skip is None else ops.add_lrelu(y, skip, JOIN_SLOPE)

    def _block(self, coefs, blk, x, pos, neighbor_idx):
        """ResNetBBlock.forward in eval mode (models/point_conv_big.py)."""
        h_in = self._mlp(coefs, blk.lin_in, x)
        skip = self._mlp(coefs, blk.shortcut, x)
        if not torch.is_tensor(pos):                       # strided block: pool the shortcut onto the coarse points
            skip = ResNetBBlock.max_pooling(skip, neighbor_idx)
        y, comb = blk.point_conv(h_in, pos, neighbor_idx, defer_combine=True)
        if comb is not None:
            comb.flush()
        return self._mlp(coefs, blk.lin_out, y, skip=skip)

    def _crf(self, coefs, d, unary, pairwise, up_idx, neighbor_idx, matrices):
        """ContinuousGaussianCRFConv.forward in eval mode (models/continuous_crf_conv_big.py)."""
        B, N, _ = pairwise.shape
        H = d.hidden_channels
        coarse, guide = unary, pairwise
        for m in d.unary_nn:
            coarse = self._mlp(coefs, m, coarse)
        for m in d.pairwise_nn:
            guide = self._mlp(coefs, m, guide)
        z = ops.gather_rows(coarse.reshape(-1, H), table_of(up_idx, unary.shape[1]))
        field = ops.crf_meanfield(z, guide.reshape(-1, H), d.c, table_of(neighbor_idx, N), d.steps, k0=1, matrices=matrices)
        refined = self._mlp(coefs, d.out_nn, field.reshape(B, N, H))
        return self._mlp(coefs, d.fusion_nn, refined, xb=pairwise)

    def _up(self, coefs, d, x_down, x_up, up_idx):
        """Upsampling.forward in eval mode (models/point_conv_big.py)."""
        return self._mlp(coefs, d.fusion, x_up, xb=self._mlp(coefs, d.lin, Upsampling.upsampling(x_down, up_idx)))

    def _forward(self, data):
        model = self.model
        ms = data.multiscale
        plan = [(model.conv1_1, ms[0].pos, ms[0].neighbor_idx), (model.conv1_2, ms[0].pos, ms[0].neighbor_idx)]
        for lvl in range(1, len(WIDTHS)):
            fine, coarse = ms[lvl - 1], ms[lvl]
            plan.append((getattr(model, 'conv%d_1' % (lvl + 1)), (fine.pos, coarse.pos), fine.sub_idx))
            plan.append((getattr(model, 'conv%d_2' % (lvl + 1)), coarse.pos, coarse.neighbor_idx))
        decoders = _decoders(model)
        crf = isinstance(decoders[0], CRFConv)
        mats = ops.crf_matrices_batched([d.c for d in decoders], ride=False) if crf else [None] * len(decoders)
        coefs = self._coefs(data.x.device)
        h = data.x
        skips = []
        for n, (blk, pos, idx) in enumerate(plan):
            if n == 4 and model.phase_hook is not None:
                model.phase_hook('coarse')
            h = self._block(coefs, blk, h, pos, idx)
            if n % 2 == 1:
                skips.append(h)                            # the level's output: the decoder's skip feature
        ops.flush_riders()
        for d, mat, lvl in zip(decoders, mats, range(len(WIDTHS) - 2, -1, -1)):
            if crf:
                h = self._crf(coefs, d, h, skips[lvl], ms[lvl].up_idx, ms[lvl].neighbor_idx, mat)
            else:
                h = self._up(coefs, d, h, skips[lvl], ms[lvl].up_idx)
        head, drop, last = model.classifier[0], model.classifier[1], model.classifier[2]
        coef = coefs.get(id(head)) if isinstance(head, MLP) else None
        if (self.fused_head and coef is not None and type(drop) is nn.Dropout
                and type(last) is nn.Linear and h.shape[-1] == head.lin.in_features and last.in_features == head.lin.out_features
                and _lib.load().crfconv_head_supported(h.numel() // h.shape[-1], head.lin.in_features, head.lin.out_features,
                                                       last.out_features)):
            # MLP -> Dropout (the identity here) -> Linear as one launch: no [M, 128] tensor
            slope = 1.0 if head.activation is None else head.activation.negative_slope
            return ops.head_eval(h, head.lin.weight, coef, slope, last.weight, last.bias).reshape(-1, model.C)
        h = drop(self._mlp(coefs, head, h))
        return ops.linear(h, last.weight, last.bias).reshape(-1, model.C)
