"""The reconstruction task network: the point-cloud autoencoder of reconstruction/src (ae_templates.py:11-43,
encoders_decoders.py:24-257, samplenet_pointnet_ae.py:57-74, 122-149) on HIP kernels.

    encoder  5 x relu(bn(conv1d_k1(.)))  3 -> 64 -> 128 -> 128 -> 256 -> bottleneck, max over the points
    decoder  relu(fc1) -> relu(fc2) -> fc3   bottleneck -> 256 -> 256 -> 3 * n_pc_points, reshaped to (B, n_pc_points, 3)

The encoder runs on the kernels of the sampler's own feature extractor (pointnet.py: the one-call conv stack in training mode where
the shape allows, sn_layer_forward_bn otherwise; sn_linear_forward + sn_bn_eval_coef in eval mode); unlike the sampler's extractor
it hands a gradient to its INPUT -- the sampler is trained through the frozen autoencoder.  Forward and backward are stack_node.py's
node around pointnet.py's layer-by-layer walk (data gradient only when frozen).  The decoder runs as the sn_skinny_linear
composition (three launches each way, row blocks of 128); weight gradients of a trainable decoder come from sn_skinny_wgrad.  A
single-launch decoder was built, lost to the composition and is NOT part of the library (profiles/ae/
decoder_single_launch_experiment.txt).  There is no CPU route.

BatchNorm follows torch: .train() = batch statistics and a running-statistics update, .eval() = running statistics.  (The reference
trains its sampler with TFLearn's is_training(True), i.e. batch statistics even in the frozen autoencoder: call .train() on the
frozen module for that behaviour, .eval() for a deterministic task network.)
"""
import numpy as np
import torch
import torch.nn as nn

from . import pointnet, stack_node
from ._lib import stream_of
from .task_features import _skinny, _skinny_wgrad, _trunk_scratch

CONV_STACK = True  # test hook: False = the encoder's training forward layer by layer at every shape


def _conv_layers(net):
    return [pointnet._Layer("conv%d" % i, getattr(net, "conv%d" % i), "bn%d" % i, getattr(net, "bn%d" % i)) for i in range(1, 6)]


class _DecoderFunction(torch.autograd.Function):
    """z (B, bottleneck) -> (B, 3 * n_pc_points): three sn_skinny_linear launches each way, in row blocks of 128 (the kernel's limit);
    weight gradients of a trainable decoder from sn_skinny_wgrad.  (A single-launch form with in-launch hand-offs of the hidden layers
    was built and measured 2.3 x SLOWER than this composition at B = 50: profiles/ae/decoder_single_launch_experiment.txt.)"""

    @staticmethod
    def forward(ctx, z, W1, b1, W2, b2, W3, b3):
        z = z.contiguous().float()
        B = z.shape[0]
        with torch.cuda.device(z.device):
            st = stream_of(z)
            h1s, h2s, outs = [], [], []
            for a in range(0, B, 128):
                zb = z[a:a + 128]
                sc = _trunk_scratch(zb.shape[0], (W1, W2, W3), z)
                h1s.append(_skinny(zb, None, W1, False, b1, True, scratch=sc, st=st))
                h2s.append(_skinny(h1s[-1], None, W2, False, b2, True, scratch=sc, st=st))
                outs.append(_skinny(h2s[-1], None, W3, False, b3, False, scratch=sc, st=st))
            h1, h2, out = (t[0] if len(t) == 1 else torch.cat(t, 0) for t in (h1s, h2s, outs))
        ctx.save_for_backward(z, h1, h2, W1, W2, W3)
        return out

    @staticmethod
    def backward(ctx, g):
        z, h1, h2, W1, W2, W3 = ctx.saved_tensors
        g = g.contiguous().float()
        B = z.shape[0]
        need = ctx.needs_input_grad
        grads = [None] * 6
        gz = None
        with torch.cuda.device(z.device):
            st = stream_of(z)
            # (row blocks of 128; the weight gradients of the blocks are added in block order)
            gzs = []
            for a in range(0, B, 128):
                s = slice(a, a + 128)
                gb, zb, h1b, h2b = g[s], z[s], h1[s], h2[s]
                sc = _trunk_scratch(gb.shape[0], (W1, W2, W3), z)
                blk = [None] * 6
                if need[5] or need[6]:
                    blk[4], blk[5] = _skinny_wgrad(h2b, None, gb, None, W3, st)
                g2 = _skinny(gb, None, W3, True, None, False, scratch=sc, st=st)
                if need[3] or need[4]:
                    blk[2], blk[3] = _skinny_wgrad(h1b, None, g2, h2b, W2, st)
                g1 = _skinny(g2, h2b, W2, True, None, False, scratch=sc, st=st)
                if need[1] or need[2]:
                    blk[0], blk[1] = _skinny_wgrad(zb, None, g1, h1b, W1, st)
                if need[0]:
                    gzs.append(_skinny(g1, h1b, W1, True, None, False, scratch=sc, st=st))
                grads = [b if a_ is None else (a_ if b is None else a_ + b) for a_, b in zip(grads, blk)]
            if need[0]:
                gz = gzs[0] if len(gzs) == 1 else torch.cat(gzs, 0)
        return (gz,) + tuple(gr if need[1 + j] else None for j, gr in enumerate(grads))


class PointNetAE(nn.Module):
    """Autoencoder of reconstruction/src/ae_templates.py:11-43 (`mlp_architecture_ala_iclr_18`): forward(x) -> (B, n_pc_points, 3).

    Parameters: conv1..conv5 (Conv1d, k = 1), bn1..bn5 (BatchNorm1d, momentum 0.1 = the reference's decay 0.9), fc1..fc3 (Linear): an
    ordinary torch state_dict.  bn_eps: TFLearn's batch_normalization epsilon -- its default is NOT in the reference tree; 1e-5 is
    recalled from TFLearn, not read: pass the value of the checkpoint's framework if it differs.
    input_shape: "bnc" (B, M, 3) or "bcn" (B, 3, M); any M (the sampler's 64 projected points, 2048 for the autoencoder's own training)."""

    def __init__(self, n_pc_points=2048, bottleneck_size=128, input_shape="bnc", bn_eps=1e-5):
        super().__init__()
        if input_shape not in ["bcn", "bnc"]:
            raise ValueError("allowed shape are 'bcn' (batch * channels * num_in_points), 'bnc' ")
        self.input_shape = input_shape
        self.n_pc_points = int(n_pc_points)
        self.bottleneck_size = int(bottleneck_size)
        widths = (3, 64, 128, 128, 256, self.bottleneck_size)
        for i in range(1, 6):
            self.add_module("conv%d" % i, nn.Conv1d(widths[i - 1], widths[i], kernel_size=1))
        for i in range(1, 6):
            self.add_module("bn%d" % i, nn.BatchNorm1d(widths[i], eps=bn_eps, momentum=0.1))
        self.fc1 = nn.Linear(self.bottleneck_size, 256)
        self.fc2 = nn.Linear(256, 256)
        self.fc3 = nn.Linear(256, 3 * self.n_pc_points)

    # captured graphs / persistent kernel scratch do not travel with a copy of the module
    _TRANSIENT = ("_sn_graphed", "_fx_acc", "_fx_acc_b")

    def __getstate__(self):
        return {k: v for k, v in self.__dict__.items() if k not in self._TRANSIENT}

    def _apply(self, fn, *args, **kwargs):
        for k in self._TRANSIENT:
            self.__dict__.pop(k, None)
        return super()._apply(fn, *args, **kwargs)

    def _check(self, t):
        if not t.is_cuda:
            raise RuntimeError("samplenet_amd.autoencoder runs on the GPU only; no CPU fallback exists")

    def encode(self, x):
        """x in `input_shape` -> (B, bottleneck): relu(bn(conv)) x 5, max over the points (encoders_decoders.py:24-131)."""
        self._check(x)
        if self.input_shape == "bcn":
            x = x.permute(0, 2, 1)
        if x.dim() != 3 or x.shape[2] != 3:
            raise RuntimeError("shape of x must be of [Batch x NumInPoints x 3] ('bnc') or [Batch x 3 x NumInPoints] ('bcn')")
        # eval mode with trainable parameters is allowed here: gradients on fixed statistics
        spec = stack_node.StackSpec(_conv_layers(self), self.training, stack_node.POOL_POINTS, self if CONV_STACK else None,
                                    stack_node.WGRADS_ASKED, None)
        return stack_node.conv_stack(spec, x.contiguous().float())[0]

    def decode(self, z):
        """z (B, bottleneck) -> (B, n_pc_points, 3): row-major reshape of the last layer's 3 * n_pc_points columns
        (samplenet_pointnet_ae.py:72-74: column 3 p + c is coordinate c of point p)."""
        self._check(z)
        out = _DecoderFunction.apply(z, self.fc1.weight, self.fc1.bias, self.fc2.weight, self.fc2.bias, self.fc3.weight, self.fc3.bias)
        return out.view(-1, self.n_pc_points, 3)

    def _forward(self, x):
        return self.decode(self.encode(x))

    def forward(self, x):
        self._check(x)
        if not self.training:
            # a frozen network on running statistics is a pure function of x: replayed from two captured graphs once the
            # configuration has been seen (graphed.py, as PCRNet); batch statistics update buffers and stay op by op
            from . import graphed

            out = graphed.call(self, "forward", self._forward, (x,))
            if out is not None:
                return out
        return self._forward(x)

    def load_tf_variables(self, mapping):
        """Fill the parameters from {TF variable name: array} with the names and shapes TFLearn gives the reference's graph:
        encoder_conv_layer_i/W (1, 1, Ci, Co) or (1, Ci, Co), /b (Co); encoder_conv_layer_i_bnorm/{gamma, beta, moving_mean,
        moving_variance}; decoder_fc_i/W (Ci, Co), /b; i from 0; scope prefixes and a ':0' suffix are ignored.  -> self."""
        got = {}
        for name, arr in mapping.items():
            parts = name.split(":")[0].split("/")
            for j in range(len(parts) - 1):
                if parts[j].startswith(("encoder_conv_layer_", "decoder_fc_")):
                    got["/".join(parts[j:j + 2])] = np.asarray(arr)
                    break

        def take(key, shape, transpose=False):
            if key not in got:
                raise KeyError("load_tf_variables: no variable %r" % key)
            a = got[key]
            if transpose:
                a = a.reshape(a.shape[-2], a.shape[-1]).T
            if tuple(a.shape) != tuple(shape):
                raise ValueError("load_tf_variables: %r has shape %s, expected %s" % (key, tuple(got[key].shape), tuple(shape)))
            return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32)

        with torch.no_grad():
            for i in range(5):
                conv, bn = getattr(self, "conv%d" % (i + 1)), getattr(self, "bn%d" % (i + 1))
                Co, Ci = conv.weight.shape[0], conv.weight.shape[1]
                conv.weight.copy_(take("encoder_conv_layer_%d/W" % i, (Co, Ci), True).view(Co, Ci, 1))
                conv.bias.copy_(take("encoder_conv_layer_%d/b" % i, (Co,)))
                for tfn, t in (("gamma", bn.weight), ("beta", bn.bias), ("moving_mean", bn.running_mean), ("moving_variance", bn.running_var)):
                    t.copy_(take("encoder_conv_layer_%d_bnorm/%s" % (i, tfn), (Co,)))
            for i in range(3):
                fc = getattr(self, "fc%d" % (i + 1))
                fc.weight.copy_(take("decoder_fc_%d/W" % i, tuple(fc.weight.shape), True))
                fc.bias.copy_(take("decoder_fc_%d/b" % i, tuple(fc.bias.shape)))
        return self


def reconstruction_loss(x_reconstr, gt, loss="chamfer"):
    """samplenet_pointnet_ae.py:125-131: "chamfer": mean(d(x_reconstr -> gt)) + mean(d(gt -> x_reconstr)); "emd": the batch mean of
    match_cost under approx_match.  Both (B, *, 3) on the GPU; the existing loss nodes of ops.py."""
    from . import ops

    if not (x_reconstr.is_cuda and gt.is_cuda):
        raise RuntimeError("samplenet_amd.autoencoder runs on the GPU only; no CPU fallback exists")
    if loss == "chamfer":
        return ops.chamfer_mean_loss(x_reconstr.contiguous(), gt.contiguous())
    if loss == "emd":
        return ops.emd_loss(x_reconstr.contiguous(), gt.contiguous()).mean()
    raise ValueError("loss: 'chamfer' or 'emd'")
