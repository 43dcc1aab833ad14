"""The classification task network: PointNet's classifier (classification/models/pointnet_cls.py:21-132, transform_nets.py:12-153,
pointnet_cls_basic.py:55-136) on HIP kernels.

    T-Net(K)   3 x relu(bn(conv1d_k1(.)))  K -> 64 -> 128 -> 1024, max over the points, 2 x relu(bn(fc))  512, 256, linear -> K * K
               (weights zero, bias the flattened identity at construction)
    PointNetCls  x . T-Net(3)(x) -> conv1, conv2 (64, 64) -> f . T-Net(64)(f) -> conv3, conv4, conv5 (64, 128, 1024) -> max over the
               points -> fc1 512 -> dropout -> fc2 256 -> dropout -> fc3 num_classes       (every conv / hidden fc: bn + relu)
    PointNetClsBasic  the same without the two T-Nets and with dropout behind fc2 only

Every conv stack runs on stack_node.py's node around pointnet.py's layer-by-layer walk (the GEMM entries of the sampler's own head;
data gradient only when the network is frozen).  The three FC heads (1024 -> 512 -> 256 -> 9 / 4096 / classes)
of a frozen network on running statistics -- the sampler-training configuration -- run as the sn_skinny_linear composition
(_SkinnyHeadFunction); on batch statistics or with trainable weights they are the N = 1 case of the same walk.  What the library had no kernel for are the
per-cloud transforms (sn_cloud_transform_*), the orthogonality regulariser (sn_orthogonality_loss_*) and the activated output of a
stack that feeds a transform instead of a GEMM (sn_bn_relu_*): csrc/cloud_transform.hip.  The gradient reaches a transformed
stack's input along several paths (through the transform's X, through the T-Net that produced T); autograd adds them in the
fixed order of the graph, which is the same every step.  There is no CPU route.

BatchNorm follows torch: .train() = batch statistics and a running-statistics update, .eval() = running statistics.  The reference
trains its sampler with the classifier in inference mode (train_samplenet.py:280,312): .eval() + requires_grad_(False) is that
configuration.  Weight gradients are produced in training mode only (every layer of an eval-mode network whose parameters ask for a
gradient raises).  Determinism: the kernels and the frozen network sum in one fixed order; the training-mode BatchNorm backward of a
stack that feeds a transform, and of a one-layer FC stack, takes its two per-channel sums from torch reductions (torch's order).
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import pointnet, stack_node
from ._lib import check, lib, ptr, stream_of


_WGRAD_NEEDS_TRAINING = stack_node.eval_wgrad_error("classifier", "network")


def _layer(mod, conv, bn, prefix=""):
    return pointnet._Layer(prefix + conv, getattr(mod, conv), prefix + bn, getattr(mod, bn))


def _stack(layers, pool, training, x):
    """relu(bn(conv1d_k1(.))) x len(layers) on x (B, N, Ci) -> (the max over the points (B, Co), argsel) when pool, else the activated
    features (B, N, Co).  Differentiable w.r.t. x and, in training mode, the layers' parameters.  An FC head is the N = 1 case."""
    spec = stack_node.StackSpec(layers, bool(training), stack_node.POOL_POINTS if pool else stack_node.POOL_NONE, None,
                                stack_node.WGRADS_ASKED, _WGRAD_NEEDS_TRAINING)
    out, argsel = stack_node.conv_stack(spec, x.contiguous().float())
    return (out, argsel) if pool else out


class _LinearFunction(torch.autograd.Function):
    """x (B, Ci) -> x W^T + b without activation (the T-Nets' `transform` layer, fc3)."""

    @staticmethod
    def forward(ctx, L, training, x, W, b):
        x = x.contiguous().float()
        with torch.cuda.device(x.device):
            z = pointnet._linear_fwd(x.shape[0], L, x, None, False)[0]
        ctx.L, ctx.x, ctx.training = L, x, bool(training)
        return z

    @staticmethod
    def backward(ctx, g):
        L, x = ctx.L, ctx.x
        g = g.contiguous().float()
        R = x.shape[0]
        gx = dW = db = None
        if (ctx.needs_input_grad[3] or ctx.needs_input_grad[4]) and not ctx.training:
            raise RuntimeError(_WGRAD_NEEDS_TRAINING)
        with torch.cuda.device(g.device):
            if ctx.needs_input_grad[3] or ctx.needs_input_grad[4]:
                dW, db = pointnet._wgrad(R, L, pointnet.DZ_PLAIN, g, None, None, None, None, 1, x, None, True)
            if ctx.needs_input_grad[2]:
                gx = pointnet._dgrad(R, L, pointnet.DZ_PLAIN, g, None, None, None, None, 1, x, None)[0]
        return None, None, gx, dW, db


def _linear(name, lin, training, x):
    return _LinearFunction.apply(pointnet._Layer(name, lin, None, None), training, x, lin.weight, lin.bias)


SKINNY_HEADS = True  # test hook: False = a frozen eval-mode FC head on the layer walk (sn_linear_forward / sn_linear_dgrad) as well


class _SkinnyHeadFunction(torch.autograd.Function):
    """A frozen FC head on running statistics, x (B, C0) -> relu(bn(fc)) x len(hidden) -> linear, as the sn_skinny_linear composition
    PCRNet's trunk and the autoencoder's decoder use (weight stream cut into column tiles x K slices; row blocks of 128): per hidden
    layer sn_skinny_linear (z = x W^T + b) and sn_bn_relu_forward with the sn_bn_eval_coef coefficients, then the last layer's
    sn_skinny_linear.  Data gradient only: sn_bn_relu_backward (mask times the BatchNorm's scale) and the transposed
    sn_skinny_linear per layer.  -> (output, the last hidden activation)."""

    @staticmethod
    def forward(ctx, hidden, last, x):
        from .task_features import _skinny, _trunk_scratch

        x = x.contiguous().float()
        B = x.shape[0]
        Ws = [L.W for L in hidden] + [last.W]
        with torch.cuda.device(x.device):
            st = stream_of(x)
            coefs = []
            for L in hidden:
                bn = L.bn
                c = torch.empty(4, L.Co, device=x.device, dtype=torch.float32)
                check(lib.sn_bn_eval_coef(L.Co, ptr(bn.weight), ptr(bn.bias), float(bn.eps), ptr(bn.running_mean), ptr(bn.running_var),
                                          ptr(c), st), "sn_bn_eval_coef")
                coefs.append(c)
            zs = [torch.empty(B, L.Co, device=x.device, dtype=torch.float32) for L in hidden]
            acts = [torch.empty(B, L.Co, device=x.device, dtype=torch.float32) for L in hidden]
            out = torch.empty(B, last.Co, device=x.device, dtype=torch.float32)
            for a in range(0, B, 128):
                r = slice(a, min(a + 128, B))
                sc = _trunk_scratch(r.stop - a, Ws, x)
                h = x[r]
                for i, L in enumerate(hidden):
                    zs[i][r] = _skinny(h, None, L.W, False, L.b, False, scratch=sc, st=st)
                    check(lib.sn_bn_relu_forward(r.stop - a, L.Co, ptr(zs[i][r]), ptr(coefs[i]), ptr(acts[i][r]), st), "sn_bn_relu_forward")
                    h = acts[i][r]
                out[r] = _skinny(h, None, last.W, False, last.b, False, scratch=sc, st=st)
        ctx.hidden, ctx.last, ctx.zs, ctx.coefs = hidden, last, zs, coefs
        return out, acts[-1]

    @staticmethod
    def backward(ctx, g, ga):
        from .task_features import _skinny, _trunk_scratch

        hidden, last, zs, coefs = ctx.hidden, ctx.last, ctx.zs, ctx.coefs
        g = g.contiguous().float()
        B = g.shape[0]
        Ws = [L.W for L in hidden] + [last.W]
        gx = torch.empty(B, hidden[0].Ci, device=g.device, dtype=torch.float32)
        with torch.cuda.device(g.device):
            st = stream_of(g)
            for a in range(0, B, 128):
                r = slice(a, min(a + 128, B))
                n = r.stop - a
                sc = _trunk_scratch(n, Ws, g)
                gh = _skinny(g[r], None, last.W, True, None, False, scratch=sc, st=st)
                if ga is not None:  # (the retrieval vectors took part in the loss themselves)
                    gh = gh + ga[r]
                for i in range(len(hidden) - 1, -1, -1):
                    L = hidden[i]
                    dz = torch.empty(n, L.Co, device=g.device, dtype=torch.float32)
                    check(lib.sn_bn_relu_backward(n, L.Co, ptr(zs[i][r]), ptr(coefs[i]), ptr(gh), 1, ptr(dz), st), "sn_bn_relu_backward")
                    gh = _skinny(dz, None, L.W, True, None, False, scratch=sc, st=st)
                gx[r] = gh
        return None, None, gx


def _head(hidden, lin_name, lin, training, x):
    """relu(bn(fc)) x len(hidden) -> linear on x (B, C0) -> (output, last hidden activation): the sn_skinny_linear composition for
    a frozen network on running statistics, pointnet.py's layer walk otherwise (batch statistics, weight gradients)."""
    last = pointnet._Layer(lin_name, lin, None, None)
    frozen = not any(p.requires_grad for p in pointnet.stack_params(hidden) + [lin.weight, lin.bias])
    if SKINNY_HEADS and not training and frozen:
        rows = min(x.shape[0], 128)
        if all(lib.sn_skinny_linear_supported(rows, L.Ci, L.Co) and lib.sn_skinny_linear_supported(rows, L.Co, L.Ci) for L in hidden + [last]):
            return _SkinnyHeadFunction.apply(hidden, last, x)
    B = x.shape[0]
    h = _stack(hidden, False, training, x.view(B, 1, -1)).view(B, -1)
    return _linear(lin_name, lin, training, h), h


class _TransformFunction(torch.autograd.Function):
    """Y[b] = X[b] . T[b] (sn_cloud_transform_forward / _backward), X (B, N, K), T (B, K, K), K in {3, 64}."""

    @staticmethod
    def forward(ctx, x, t):
        x, t = x.contiguous().float(), t.contiguous().float()
        B, N, K = x.shape
        y = torch.empty_like(x)
        with torch.cuda.device(x.device):
            check(lib.sn_cloud_transform_forward(B, N, K, ptr(x), ptr(t), ptr(y), stream_of(x)), "sn_cloud_transform_forward")
        ctx.save_for_backward(x, t)
        return y

    @staticmethod
    def backward(ctx, g):
        x, t = ctx.saved_tensors
        B, N, K = x.shape
        g = g.contiguous().float()
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dt = torch.empty_like(t) if ctx.needs_input_grad[1] else None
        with torch.cuda.device(x.device):
            check(lib.sn_cloud_transform_backward(B, N, K, ptr(x), ptr(t), ptr(g), ptr(dx), ptr(dt), stream_of(x)),
                  "sn_cloud_transform_backward")
        return dx, dt


def cloud_transform(x, t):
    """Every cloud's rows times that cloud's own matrix: x (B, N, K) . t (B, K, K), K = 3 or 64; differentiable in both."""
    if not (x.is_cuda and t.is_cuda):
        raise RuntimeError("samplenet_amd.classifier runs on the GPU only; no CPU fallback exists")
    if x.dim() != 3 or t.dim() != 3 or x.shape[2] not in (3, 64) or tuple(t.shape) != (x.shape[0], x.shape[2], x.shape[2]):
        raise RuntimeError("cloud_transform: x (B, N, K), t (B, K, K), K = 3 or 64")
    return _TransformFunction.apply(x, t)


class _OrthogonalityFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t):
        t = t.contiguous().float()
        B, K, _ = t.shape
        partial = torch.empty(max(B, 1), device=t.device, dtype=torch.float32)
        loss = torch.zeros((), device=t.device, dtype=torch.float32)
        with torch.cuda.device(t.device):
            check(lib.sn_orthogonality_loss_forward(B, K, ptr(t), ptr(partial), ptr(loss), stream_of(t)), "sn_orthogonality_loss_forward")
        ctx.save_for_backward(t)
        return loss

    @staticmethod
    def backward(ctx, g):
        (t,) = ctx.saved_tensors
        B, K, _ = t.shape
        g = g.contiguous().float()
        dt = torch.zeros_like(t) if B == 0 else torch.empty_like(t)
        with torch.cuda.device(t.device):
            check(lib.sn_orthogonality_loss_backward(B, K, ptr(t), ptr(g), ptr(dt), stream_of(t)), "sn_orthogonality_loss_backward")
        return dt


def orthogonality_loss(t):
    """tf.nn.l2_loss(T T^T - I) of pointnet_cls.py:124-130: 1/2 sum over the batch of |T[b] T[b]^T - I|^2; t (B, K, K), K = 3 or 64."""
    if not t.is_cuda:
        raise RuntimeError("samplenet_amd.classifier runs on the GPU only; no CPU fallback exists")
    if t.dim() != 3 or t.shape[1] != t.shape[2] or t.shape[1] not in (3, 64):
        raise RuntimeError("orthogonality_loss: t (B, K, K), K = 3 or 64")
    return _OrthogonalityFunction.apply(t)


class _TNet(nn.Module):
    """input_transform_net / feature_transform_net of transform_nets.py:12-153: (B, N, K) -> (B, K, K).  The last layer starts with
    zero weights and the flattened identity as bias (transform_nets.py:59-66, 134-141)."""

    def __init__(self, K, bn_eps):
        super().__init__()
        self.K = K
        widths = (K, 64, 128, 1024)
        for i in range(1, 4):
            self.add_module("tconv%d" % i, nn.Conv1d(widths[i - 1], widths[i], kernel_size=1))
            self.add_module("bn%d" % i, nn.BatchNorm1d(widths[i], eps=bn_eps, momentum=0.1))
        self.tfc1, self.bn4 = nn.Linear(1024, 512), nn.BatchNorm1d(512, eps=bn_eps, momentum=0.1)
        self.tfc2, self.bn5 = nn.Linear(512, 256), nn.BatchNorm1d(256, eps=bn_eps, momentum=0.1)
        self.transform = nn.Linear(256, K * K)
        with torch.no_grad():
            self.transform.weight.zero_()
            self.transform.bias.copy_(torch.eye(K).flatten())

    def run(self, x, prefix):
        B = x.shape[0]
        convs = [_layer(self, "tconv%d" % i, "bn%d" % i, prefix) for i in range(1, 4)]
        fcs = [_layer(self, "tfc1", "bn4", prefix), _layer(self, "tfc2", "bn5", prefix)]
        pooled, _ = _stack(convs, True, self.training, x)
        return _head(fcs, prefix + "transform", self.transform, self.training, pooled)[0].view(B, self.K, self.K)


class PointNetCls(nn.Module):
    """PointNet's classifier (pointnet_cls.py:21-114): forward(x) -> (logits (B, num_classes), end_points) with end_points
    `transform` (B, 64, 64), `critical_set_idx` (B, 1024) int32, `GFV` (B, 1024), `retrieval_vectors` (B, 256).

    Parameters, an ordinary torch state_dict: transform_net1 / transform_net2 (.tconv1..3, .tfc1, .tfc2, .transform, .bn1..bn5 = the
    BatchNorms of tconv1..3, tfc1, tfc2), conv1..conv5 with bn1..bn5, fc1, fc2 with bn_fc1, bn_fc2, fc3.  BatchNorm epsilon 1e-3 and
    momentum 0.1 (tf_util.py:500,518: decay 0.9).  input_shape: "bnc" (B, N, 3) or "bcn" (B, 3, N); any N."""

    transforms = True
    dropouts = (True, True)

    def __init__(self, num_classes=40, input_shape="bnc", bn_eps=1e-3, dropout=0.3):
        super().__init__()
        if input_shape not in ["bcn", "bnc"]:
            raise ValueError("allowed shape are 'bcn' (batch * channels * num_in_points), 'bnc' ")
        self.input_shape = input_shape
        self.num_classes = int(num_classes)
        self.dropout = float(dropout)
        if self.transforms:
            self.transform_net1 = _TNet(3, bn_eps)
        widths = (3, 64, 64, 64, 128, 1024)
        for i in range(1, 6):
            self.add_module("conv%d" % i, nn.Conv1d(widths[i - 1], widths[i], kernel_size=1))
            self.add_module("bn%d" % i, nn.BatchNorm1d(widths[i], eps=bn_eps, momentum=0.1))
            if i == 2 and self.transforms:
                self.transform_net2 = _TNet(64, bn_eps)
        self.fc1, self.bn_fc1 = nn.Linear(1024, 512), nn.BatchNorm1d(512, eps=bn_eps, momentum=0.1)
        self.fc2, self.bn_fc2 = nn.Linear(512, 256), nn.BatchNorm1d(256, eps=bn_eps, momentum=0.1)
        self.fc3 = nn.Linear(256, self.num_classes)

    def _drop(self, h, on):
        # 32 rows: a torch-generated mask (F.dropout scales the kept activations by 1 / (1 - p)); identity in eval mode
        return F.dropout(h, self.dropout, True) if on and self.training and self.dropout > 0 else h

    def forward(self, x):
        if not x.is_cuda:
            raise RuntimeError("samplenet_amd.classifier runs on the GPU only; no CPU fallback exists")
        if self.input_shape == "bcn":
            x = x.permute(0, 2, 1)
        if x.dim() != 3 or x.shape[2] != 3:
            raise RuntimeError("shape of x must be of [Batch x NumInPoints x 3] ('bnc') or [Batch x 3 x NumInPoints] ('bcn')")
        x = x.contiguous().float()
        B = x.shape[0]
        tr = self.training
        end_points = {}
        convs = [_layer(self, "conv%d" % i, "bn%d" % i) for i in range(1, 6)]
        if self.transforms:
            x = cloud_transform(x, self.transform_net1.run(x, "transform_net1."))
            f = _stack(convs[:2], False, tr, x)
            t2 = self.transform_net2.run(f, "transform_net2.")
            end_points["transform"] = t2
            pooled, argsel = _stack(convs[2:], True, tr, cloud_transform(f, t2))
        else:
            pooled, argsel = _stack(convs, True, tr, x)
        end_points["critical_set_idx"] = argsel
        end_points["GFV"] = pooled
        fc1, fc2 = _layer(self, "fc1", "bn_fc1"), _layer(self, "fc2", "bn_fc2")
        if tr and self.dropout > 0:
            # a torch-generated mask behind fc1 (full model) and fc2: one-layer stacks with the mask between them
            h = self._drop(_stack([fc1], False, tr, pooled.view(B, 1, -1)), self.dropouts[0])
            h = self._drop(_stack([fc2], False, tr, h).view(B, -1), self.dropouts[1])
            logits = _linear("fc3", self.fc3, tr, h)
        else:
            logits, h = _head([fc1, fc2], "fc3", self.fc3, tr, pooled)
        end_points["retrieval_vectors"] = h
        return logits, end_points


class PointNetClsBasic(PointNetCls):
    """pointnet_cls_basic.py:55-136: the classifier without T-Nets, dropout behind fc2 only; end_points has no `transform`."""

    transforms = False
    dropouts = (False, True)


def classification_loss(logits, labels, end_points, reg_weight=0.001, fused=False):
    """pointnet_cls.py:117-132: mean softmax cross-entropy + reg_weight * l2_loss(T T^T - I) of end_points["transform"] (absent for
    the basic model: cross-entropy alone, pointnet_cls_basic.py:139-146).  labels: (B,) integer class indices on the GPU.
    fused=True: the cross-entropy is ops.classification_terms' means[0] (through ops.classification_mean_loss, which hands the
    upstream scalar straight to the backward entry) -- one HIP launch each way (sn_classification_terms_*)
    instead of torch's log-softmax / NLL kernels; the default stays F.cross_entropy."""
    if not (logits.is_cuda and labels.is_cuda):
        raise RuntimeError("samplenet_amd.classifier runs on the GPU only; no CPU fallback exists")
    if fused:
        from . import ops

        loss = ops.classification_mean_loss(logits, labels)  # (= ops.classification_terms(logits, labels)[3][0])
    else:
        loss = F.cross_entropy(logits, labels.long())
    t = end_points.get("transform")
    if t is not None:
        loss = loss + reg_weight * orthogonality_loss(t)
    return loss
