"""Restatement of PointNet's classifier in plain torch.nn layers, written from the reference's lines
(classification/models/pointnet_cls.py:21-132, transform_nets.py:12-153, pointnet_cls_basic.py:55-146): the yardstick of
tests/test_gpu_classifier.py (in fp32 on the device and as .double()) and of tests/test_classifier_host.py (strict state_dict load).
The reference itself is TensorFlow and cannot run beside these tests."""
import torch
import torch.nn as nn
import torch.nn.functional as F


class TorchTNet(nn.Module):
    def __init__(self, K, bn_eps):
        super().__init__()
        self.K = K
        widths = (K, 64, 128, 1024)  # transform_nets.py:21-43 / 95-117
        for i in range(1, 4):
            setattr(self, "tconv%d" % i, nn.Conv1d(widths[i - 1], widths[i], 1))
            setattr(self, "bn%d" % i, nn.BatchNorm1d(widths[i], eps=bn_eps, momentum=0.1))
        self.tfc1, self.bn4 = nn.Linear(1024, 512), nn.BatchNorm1d(512, eps=bn_eps, momentum=0.1)
        self.tfc2, self.bn5 = nn.Linear(512, 256), nn.BatchNorm1d(256, eps=bn_eps, momentum=0.1)
        self.transform = nn.Linear(256, K * K)  # transform_nets.py:59-72: zero weights, identity bias

    def forward(self, x):  # (B, K, N)
        for i in range(1, 4):
            x = F.relu(getattr(self, "bn%d" % i)(getattr(self, "tconv%d" % i)(x)))
        x = x.max(dim=2)[0]
        x = F.relu(self.bn4(self.tfc1(x)))
        x = F.relu(self.bn5(self.tfc2(x)))
        return self.transform(x).view(-1, self.K, self.K)


class TorchCls(nn.Module):
    def __init__(self, num_classes=40, bn_eps=1e-3, dropout=0.3, basic=False):
        super().__init__()
        self.basic, self.p = basic, dropout
        if not basic:
            self.transform_net1 = TorchTNet(3, bn_eps)
        widths = (3, 64, 64, 64, 128, 1024)
        for i in range(1, 6):
            setattr(self, "conv%d" % i, nn.Conv1d(widths[i - 1], widths[i], 1))
            setattr(self, "bn%d" % i, nn.BatchNorm1d(widths[i], eps=bn_eps, momentum=0.1))
            if i == 2 and not basic:
                self.transform_net2 = TorchTNet(64, bn_eps)
        self.fc1, self.bn_fc1 = nn.Linear(1024, 512), nn.BatchNorm1d(512, eps=bn_eps, momentum=0.1)
        self.fc2, self.bn_fc2 = nn.Linear(512, 256), nn.BatchNorm1d(256, eps=bn_eps, momentum=0.1)
        self.fc3 = nn.Linear(256, num_classes)

    def _conv(self, i, x):
        return F.relu(getattr(self, "bn%d" % i)(getattr(self, "conv%d" % i)(x)))

    def forward(self, x):  # (B, N, 3)
        end_points = {}
        if not self.basic:
            x = torch.bmm(x, self.transform_net1(x.permute(0, 2, 1)))  # pointnet_cls.py:27-29
        f = self._conv(2, self._conv(1, x.permute(0, 2, 1)))
        if not self.basic:
            t = self.transform_net2(f)  # pointnet_cls.py:55-58
            end_points["transform"] = t
            f = torch.bmm(f.permute(0, 2, 1), t).permute(0, 2, 1)
        f = self._conv(5, self._conv(4, self._conv(3, f)))
        end_points["pre_pool"] = f  # (B, 1024, N): what critical_set_idx is the argmax of
        end_points["critical_set_idx"] = f.argmax(dim=2)  # pointnet_cls.py:95
        g = f.max(dim=2)[0]
        end_points["GFV"] = g
        h = F.relu(self.bn_fc1(self.fc1(g)))
        if not self.basic:
            h = F.dropout(h, self.p, self.training)  # pointnet_cls.py:105 (the basic model has no dp1)
        h = F.dropout(F.relu(self.bn_fc2(self.fc2(h))), self.p, self.training)
        end_points["retrieval_vectors"] = h
        return self.fc3(h), end_points


def torch_classification_loss(logits, labels, end_points, reg_weight=0.001):
    """pointnet_cls.py:117-132."""
    loss = F.cross_entropy(logits, labels)
    t = end_points.get("transform")
    if t is not None:
        d = torch.bmm(t, t.transpose(1, 2)) - torch.eye(t.shape[1], dtype=t.dtype, device=t.device)
        loss = loss + reg_weight * 0.5 * (d * d).sum()
    return loss


def torch_cls_copy(state_dict, num_classes=40, bn_eps=1e-3, dropout=0.3, basic=False, dtype=torch.float32, device=None):
    """TorchCls carrying a PointNetCls.state_dict() (strict)."""
    m = TorchCls(num_classes, bn_eps, dropout, basic)
    m.load_state_dict({k: v.detach().clone().cpu() for k, v in state_dict.items()}, strict=True)
    m = m.to(dtype)
    return m.to(device) if device is not None else m
