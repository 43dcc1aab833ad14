"""Restatement of the reconstruction autoencoder in plain torch.nn layers, written from the reference's lines
(reconstruction/src/ae_templates.py:11-43, encoders_decoders.py:24-257, samplenet_pointnet_ae.py:57-74): the yardstick of
tests/test_gpu_autoencoder.py (in fp32 on the device and as .double()) and of tests/test_autoencoder_host.py (CPU, fp64).
The reference itself is TensorFlow / TFLearn and cannot run beside these tests."""
import torch
import torch.nn as nn
import torch.nn.functional as F


class TorchAE(nn.Module):
    def __init__(self, n_pc_points=2048, bottleneck_size=128, input_shape="bnc", bn_eps=1e-5):
        super().__init__()
        self.n_pc_points, self.input_shape = n_pc_points, input_shape
        widths = (3, 64, 128, 128, 256, bottleneck_size)  # ae_templates.py:27: n_filters = [64, 128, 128, 256, bneck]
        for i in range(1, 6):
            setattr(self, "conv%d" % i, nn.Conv1d(widths[i - 1], widths[i], 1))
        for i in range(1, 6):
            setattr(self, "bn%d" % i, nn.BatchNorm1d(widths[i], eps=bn_eps, momentum=0.1))
        self.fc1 = nn.Linear(bottleneck_size, 256)  # ae_templates.py:36: layer_sizes = [256, 256, n_pc_points * 3]
        self.fc2 = nn.Linear(256, 256)
        self.fc3 = nn.Linear(256, 3 * n_pc_points)

    def encode(self, x):
        if self.input_shape == "bnc":
            x = x.permute(0, 2, 1)
        for i in range(1, 6):  # encoders_decoders.py:96-118: conv -> batch norm -> relu, the last layer included
            x = F.relu(getattr(self, "bn%d" % i)(getattr(self, "conv%d" % i)(x)))
        return x.max(dim=2)[0]  # encoders_decoders.py:120-121: symmetry = reduce_max over the points

    def decode(self, z):
        z = F.relu(self.fc1(z))  # encoders_decoders.py:160-185: fully connected -> relu, twice
        z = F.relu(self.fc2(z))
        return self.fc3(z).view(-1, self.n_pc_points, 3)  # last layer linear; samplenet_pointnet_ae.py:72-74 reshape

    def forward(self, x):
        return self.decode(self.encode(x))


def torch_ae_copy(state_dict, n_pc_points=2048, bottleneck_size=128, input_shape="bnc", bn_eps=1e-5, dtype=torch.float32, device=None):
    """TorchAE carrying a PointNetAE.state_dict()."""
    m = TorchAE(n_pc_points, bottleneck_size, input_shape, bn_eps)
    m.load_state_dict({k: v.detach().clone().cpu() for k, v in state_dict.items()})
    m = m.to(dtype)
    return m.to(device) if device is not None else m
