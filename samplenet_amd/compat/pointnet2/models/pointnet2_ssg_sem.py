"""PointNet2SemSegSSG: the single-scale PointNet++ segmentation network -- four set-abstraction levels down, four
feature-propagation levels up, a two-layer per-point head -- joined from the modules of pointnet2_modules.

    net = PointNet2SemSegSSG(num_classes, input_channels=0, use_xyz=True, fused=True)
    logits = net(xyz (B,N,3), features (B,input_channels,N) or None)      # (B, num_classes, N)

The logits are returned in the original's shape (B, num_classes, N), which F.cross_entropy takes as it is, and their MEMORY is
(B, N, num_classes): the return value is a transposed view of the head's rows, which segmentation_loss / ops.segmentation_terms
read without a copy.

fused=True: the feature-propagation levels run their fused route (row layout, HIP GEMM walk) and hand each other transposed views;
the head reads the last level's rows view without a copy.  The set-abstraction levels run their fused route either way (their own
default).  The head itself is torch: its weights are kept in Conv1d shape (state_dict compatible with a Conv1d head) and applied
with F.linear on the rows; BatchNorm1d and Dropout act on the (B * N, width) rows.

The level tables are constructor data:
    sa   = ((npoint, radius, nsample, (widths..)), ..)   four levels, widths WITHOUT the input width
    fp   = ((widths..), ..)                              four levels, fp[0] the finest (its output feeds the head)
    head = hidden width of the head
The defaults are the original's single-scale segmentation network AS RECALLED; like the rest of this package the constructor
arguments and the state_dict key names (SA_modules.<i>.., FP_modules.<i>.., fc_layer.<0|1|4>..) are UNPINNED."""
import torch.nn.functional as F
from torch import nn

from ..utils.pointnet2_modules import PointnetFPModule, PointnetSAModule, _rows_of

SA_DEFAULT = ((1024, 0.1, 32, (32, 32, 64)), (256, 0.2, 32, (64, 64, 128)), (64, 0.4, 32, (128, 128, 256)),
              (16, 0.8, 32, (256, 256, 512)))
FP_DEFAULT = ((128, 128, 128), (256, 128), (256, 256), (256, 256))
HEAD_DEFAULT = 128


class PointNet2SemSegSSG(nn.Module):
    def __init__(self, num_classes, input_channels=0, use_xyz=True, fused=True, sa=SA_DEFAULT, fp=FP_DEFAULT, head=HEAD_DEFAULT):
        super().__init__()
        if len(sa) != len(fp):
            raise ValueError("PointNet2SemSegSSG: one feature-propagation level per set-abstraction level")
        self.fused = bool(fused)
        self.SA_modules = nn.ModuleList()
        skips = [int(input_channels)]  # feature width at every resolution, the input's first
        for npoint, radius, nsample, widths in sa:
            self.SA_modules.append(PointnetSAModule([skips[-1]] + list(widths), npoint=npoint, radius=radius, nsample=nsample,
                                                    use_xyz=use_xyz))
            skips.append(int(widths[-1]))
        self.FP_modules = nn.ModuleList()
        below = [int(w[-1]) for w in fp[1:]] + [skips[-1]]  # what comes up into level j: level j + 1's output, the deepest SA's at the end
        for j, widths in enumerate(fp):
            self.FP_modules.append(PointnetFPModule([below[j] + skips[j]] + list(widths), fused=self.fused))
        self.fc_layer = nn.Sequential(nn.Conv1d(int(fp[0][-1]), int(head), kernel_size=1, bias=False), nn.BatchNorm1d(int(head)),
                                      nn.ReLU(True), nn.Dropout(0.5), nn.Conv1d(int(head), int(num_classes), kernel_size=1))

    def head_rows(self, rows):
        """rows (B,N,W) -> logits (B,N,num_classes): the Conv1d weights applied as F.linear on the rows."""
        conv0, bn, act, drop, conv1 = self.fc_layer
        B, N, W = rows.shape
        x = F.linear(rows.reshape(B * N, W), conv0.weight.squeeze(-1))
        x = drop(act(bn(x)))
        return F.linear(x, conv1.weight.squeeze(-1), conv1.bias).view(B, N, -1)

    def forward(self, xyz, features=None):
        l_xyz, l_features = [xyz], [features]
        for sa in self.SA_modules:
            li_xyz, li_features = sa(l_xyz[-1], l_features[-1])
            l_xyz.append(li_xyz)
            l_features.append(li_features)
        for i in range(-1, -(len(self.FP_modules) + 1), -1):
            l_features[i - 1] = self.FP_modules[i](l_xyz[i - 1], l_xyz[i], l_features[i - 1], l_features[i])
        return self.head_rows(_rows_of(l_features[0])).transpose(1, 2)
