"""task_features.pcrnet_loss / sampling_consistency (registration/main.py:540-598 with `--loss-type 0`) and the captured training
step that carries them: B = 4 clouds of N = 128 points, a PCRNet with default initialisation under a fixed seed."""
import copy

import numpy as np
import pytest
import torch

import pose_ref as P
from torch_mlp import rel as _rel

pytestmark = pytest.mark.gpu

B, N = 4, 128
INFO_KEYS = {"chamfer_loss", "qnorm_loss", "rot_err", "norm_err", "trans_err", "est_transform"}  # main.py:589-596


def _data(seed=3):
    g = torch.Generator().manual_seed(seed)
    p0 = (torch.rand(B, N, 3, generator=g) - 0.5).cuda()
    est, gt = P.make_case("unit", B)
    igt = torch.from_numpy(gt).cuda()
    from samplenet_amd.task_features import qrot_cloud

    p1 = qrot_cloud(igt[:, :4].contiguous(), p0) + 0.01 * (torch.rand(B, N, 3, generator=g) - 0.5).cuda()
    return p0, p1.detach(), igt


def _pcrnet(frozen, seed=21):
    from samplenet_amd.task_features import PCRNet

    torch.manual_seed(seed)
    model = PCRNet(bottleneck_size=256, input_shape="bnc").cuda()
    if frozen:
        model.eval()
        for p in model.parameters():
            p.requires_grad_(False)
    return model


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def reference_loss(model, p0, p1, igt, loss_type):
    """compute_pcrnet_loss (main.py:557-598) restated in fp64 torch on the model's weights: PointNetFeatures (five 1x1 convolutions with
    ReLU, max over the points), the six-layer trunk, F.normalize, qrot, the Chamfer means, the pose terms of tests/pose_ref.py."""
    p0, p1 = p0.double(), p1.double()

    def feat(x):
        h = x
        for conv in (model.feat.conv1, model.feat.conv2, model.feat.conv3, model.feat.conv4, model.feat.conv5):
            h = torch.relu(h @ conv.weight.double().squeeze(-1).t() + conv.bias.double())
        return h.max(1)[0]

    y = torch.cat([feat(p0), feat(p1)], dim=1)
    fcs = (model.fc1, model.fc2, model.fc3, model.fc4, model.fc5, model.fc6)
    for i, fc in enumerate(fcs):
        y = y @ fc.weight.double().t() + fc.bias.double()
        if i < 5:
            y = torch.relu(y)
    pre = y[:, :4]
    q = pre / pre.norm(dim=1, keepdim=True).clamp_min(1e-12)
    twist = torch.cat([q, y[:, 4:]], dim=1)
    qv = q[:, None, 1:].expand(-1, p0.shape[1], -1)
    uv = torch.cross(qv, p0, dim=-1)
    p1_est = p0 + 2 * (q[:, None, :1] * uv + torch.cross(qv, uv, dim=-1))
    d = ((p1[:, :, None] - p1_est[:, None]) ** 2).sum(-1)
    chamfer = d.min(2)[0].mean() + d.min(1)[0].mean()
    rot, nrm, trn = P.pose_terms_torch(twist, igt)
    loss = 1.0 * nrm.mean() + 1.0 * chamfer if loss_type == 0 else chamfer
    return loss, {"chamfer_loss": chamfer, "qnorm_loss": ((pre ** 2).sum(1) - 1).pow(2).mean(), "rot_err": rot.mean() * 180 / np.pi,
                  "norm_err": nrm.mean(), "trans_err": trn.mean(), "twist": twist}


def test_loss_type_1_is_pcrnet_chamfer_loss_and_type_0_adds_norm_err():
    from samplenet_amd import QuaternionTransform
    from samplenet_amd.task_features import pcrnet_chamfer_loss, pcrnet_loss

    model = _pcrnet(frozen=False)
    p0, p1, igt = _data()
    want, qn, twist = pcrnet_chamfer_loss(model, p0, p1)
    loss1, info1 = pcrnet_loss(model, p0, p1, igt, loss_type=1)
    assert torch.equal(_bits(loss1), _bits(want)) and torch.equal(_bits(info1["est_transform"].vec), _bits(twist))
    assert torch.equal(_bits(info1["qnorm_loss"]), _bits(qn)) and torch.equal(_bits(info1["chamfer_loss"]), _bits(want))
    loss0, info0 = pcrnet_loss(model, p0, p1, {"vec": igt.cpu(), "inversion": torch.tensor([False])})  # the reference's dict, default type 0
    assert set(info0) == set(info1) == INFO_KEYS
    r, n, t = QuaternionTransform(twist).compute_errors(QuaternionTransform(igt))
    assert torch.equal(_bits(loss0), _bits(n + want))
    assert torch.equal(_bits(info0["norm_err"]), _bits(n)) and torch.equal(_bits(info0["trans_err"]), _bits(t))
    assert torch.equal(_bits(info0["rot_err"]), _bits(r * (180 / np.pi)))  # degrees
    assert not info0["rot_err"].requires_grad and info0["norm_err"].requires_grad
    # want_info=False (what a captured step asks for): the same loss, no info, nothing launched for the metrics alone
    for lt, want_loss in ((0, loss0), (1, loss1)):
        lv, none = pcrnet_loss(model, p0, p1, igt, loss_type=lt, want_info=False)
        assert none is None and torch.equal(_bits(lv), _bits(want_loss)), lt
    with pytest.raises(ValueError):
        pcrnet_loss(model, p0, p1, igt, loss_type=2)


@pytest.mark.parametrize("loss_type", [0, 1])
def test_values_and_gradients_against_fp64(loss_type):
    """Loss, info and the gradients to a TRAINABLE PCRNet's parameters and to p1 against the fp64 restatement.  The bar is the one
    tests/test_gpu_mlp.py::test_pcrnet_task_loss_matches_reference sets for the Chamfer term of this network: values within 1e-5
    (relative above 1), every gradient within 2e-4 of the reference gradient's norm (torch_mlp.rel)."""
    from samplenet_amd.task_features import pcrnet_loss

    model = _pcrnet(frozen=False)
    p0, p1, igt = _data()
    p1 = p1.clone().requires_grad_(True)
    loss, info = pcrnet_loss(model, p0, p1, igt, loss_type=loss_type)
    params = dict(model.named_parameters())
    got = torch.autograd.grad(loss, [p1] + list(params.values()))
    p1r = p1.detach().clone().requires_grad_(True)
    rloss, rinfo = reference_loss(model, p0, p1r, igt, loss_type)
    want = torch.autograd.grad(rloss, [p1r] + list(params.values()))
    close = lambda a, b: abs(float(a.detach()) - float(b.detach())) <= 1e-5 * max(1.0, abs(float(b.detach())))  # noqa: E731
    assert close(loss, rloss)
    for k in ("chamfer_loss", "qnorm_loss", "norm_err", "trans_err"):
        assert close(info[k], rinfo[k]), k
    assert torch.allclose(info["est_transform"].vec.detach().double(), rinfo["twist"], rtol=1e-5, atol=1e-6)
    # rot_err (degrees) against the fp64 terms of the network's OWN fp32 twist, under pose_ref's counted bound (+ the conversion's
    # rounding); acos' condition makes a comparison across the fp32 / fp64 networks meaningless near the ends
    T = P.pose_terms(info["est_transform"].vec.detach().cpu().numpy(), igt.cpu().numpy())
    assert np.isfinite(float(info["rot_err"]))
    if P.rot_admitted(T).all():
        deg = 180 / np.pi
        assert abs(float(info["rot_err"]) - T["rot_err"].mean() * deg) <= (P.bound_mean(B, T["rot_err"], P.bound_rot_err(T)) * deg
                                                                           + 2 * P.U * float(info["rot_err"]))
    for name, a, b in zip(["p1"] + list(params), got, want):
        assert _rel(a, b) <= 2e-4, (name, _rel(a, b))


def test_frozen_network_replays_captured_graphs_bit_for_bit():
    from samplenet_amd import graphed
    from samplenet_amd.task_features import pcrnet_loss

    pcr = _pcrnet(frozen=True)
    ref = copy.deepcopy(pcr)
    ref.graph_surface = False
    g = torch.Generator(device="cuda").manual_seed(12)
    _, _, igt = _data()
    for i in range(4):
        p0 = torch.rand(B, N, 3, device="cuda", generator=g) - 0.5
        q = torch.rand(B, 64, 3, device="cuda", generator=g) - 0.5
        res = []
        for net in (pcr, ref):
            qq = q.clone().requires_grad_(True)
            loss, info = pcrnet_loss(net, p0, qq, igt)
            (loss + 0.3 * info["qnorm_loss"] + 0.5 * info["trans_err"]).backward()
            res.append([t.detach().clone() for t in (loss, info["chamfer_loss"], info["qnorm_loss"], info["rot_err"], info["norm_err"],
                                                     info["trans_err"], info["est_transform"].vec, qq.grad)])
        for u, v in zip(*res):
            assert torch.equal(_bits(u), _bits(v)), i
        plans = [p for k, p in pcr.__dict__.get("_sn_graphed", {}).items() if isinstance(p, graphed._Plan) and k[0] == "pcrnet_loss0"]
        assert (len(plans) == 1) == (i >= 2), i
    assert not any(isinstance(p, graphed._Plan) for p in ref.__dict__.get("_sn_graphed", {}).values())


def test_sampling_consistency():
    """main.py:540-555: zero for a source that IS the rotated template; otherwise the Chamfer mean of p0 against the source rotated
    back, here against fp64 within the Chamfer term's own 1e-5 bar."""
    from samplenet_amd.task_features import qrot_cloud, sampling_consistency

    p0, p1, igt = _data()
    exact = qrot_cloud(igt[:, :4].contiguous(), p0)
    assert float(sampling_consistency(p0, exact, igt)) <= 1e-12  # (squared distances of ~1e-7 displacements)
    got = sampling_consistency(p0, p1, {"vec": igt, "inversion": torch.tensor([False])})
    q = igt[:, :4].double() * torch.tensor([1.0, -1, -1, -1], dtype=torch.float64, device="cuda")
    qv = q[:, None, 1:].expand(-1, N, -1)
    uv = torch.cross(qv, p1.double(), dim=-1)
    back = p1.double() + 2 * (q[:, None, :1] * uv + torch.cross(qv, uv, dim=-1))
    d = ((p0.double()[:, :, None] - back[:, None]) ** 2).sum(-1)
    want = d.min(2)[0].mean() + d.min(1)[0].mean()
    assert abs(float(got) - float(want)) <= 1e-5 * max(1.0, float(want)) and float(want) > 0


# ------------------------------------------------------------------------------------------------ the captured step
EB, EN, EM = 4, 128, 8


def _set():
    g = torch.Generator().manual_seed(2)
    return (torch.rand(8, 130, 3, generator=g) - 0.5).cuda(), torch.arange(8).cuda()


def _nets(n):
    from samplenet_amd import SampleNet

    torch.manual_seed(0)
    mk = lambda: SampleNet(EM, 128, group_size=4, initial_temperature=1.0, input_shape="bnc", output_shape="bnc").cuda().train()  # noqa: E731
    nets = [mk()]
    sd = copy.deepcopy(nets[0].state_dict())
    for _ in range(n - 1):
        nets.append(mk())
        nets[-1].load_state_dict(sd)
    return nets


def test_captured_step_carries_loss_type_0():
    """SamplerTrainStep(task_loss_igt=True) on a pair-making source: the source's one launch fills x, x1 and igt; the captured step
    equals the eager one bit for bit over three steps (loss and every gradient), and the igt it saw is source.at(position)'s."""
    from samplenet_amd import BatchRecipe, DeviceBatchSource, DeviceCloudSet
    from samplenet_amd.engine import SamplerTrainStep
    from samplenet_amd.parallel import FlatGradAllReducer
    from samplenet_amd.task_features import pcrnet_loss

    pts, labels = _set()
    rc = BatchRecipe(shuffle_points=True, unit_cube=True)
    mk = lambda: DeviceBatchSource(DeviceCloudSet(pts, labels), rc, EB, EN, seed=6, pair="fixed")  # noqa: E731
    want = mk().at(0)
    pcr = _pcrnet(frozen=True, seed=1)
    seen = []

    def task(proj, p1, igt):  # template = the sampled cloud, source = p1 (as tests/test_gpu_batch_assemble.py's pair test)
        seen.append(igt)
        return pcrnet_loss(pcr, proj, p1, igt, loss_type=0, want_info=False)[0]

    na, nb = _nets(2)
    ra, rb = FlatGradAllReducer(na), FlatGradAllReducer(nb)
    sa = SamplerTrainStep(na, want.p0, reducer=ra, task_loss=task, input_source=mk(), task_loss_igt=True)
    sb = SamplerTrainStep(nb, want.p0, reducer=rb, task_loss=task, input_source=mk(), task_loss_igt=True, use_graph=False)
    assert len(sa._ring_graphs[0]) == 1 and not sb._ring_graphs and all(t is sa.igt or t is sb.igt for t in seen)
    losses = []
    for i in range(3):
        la, lb = sa.step(), sb.step()
        torch.cuda.synchronize()
        batch = mk().at(i * EB)
        for s in (sa, sb):
            assert torch.equal(_bits(s.igt), _bits(batch.igt)) and torch.equal(_bits(s.x1), _bits(batch.p1)) and torch.equal(_bits(s.x), _bits(batch.p0)), i
        assert torch.equal(_bits(la), _bits(lb)) and torch.isfinite(la) and torch.equal(_bits(ra.flat), _bits(rb.flat)), i
        assert float(ra.flat.abs().sum()) > 0
        losses.append(float(la))
    assert len(set(losses)) == 3 and sa.source.position == 3 * EB
    with pytest.raises(ValueError):
        SamplerTrainStep(na, want.p0, task_loss=task, task_loss_igt=True)  # no pair-making source


def test_two_argument_task_loss_is_unchanged():
    """The unchanged-behaviour guard: without task_loss_igt a pair-making source still calls task_loss(proj, x1), fills no igt, and
    gives the numbers of the same step fed the same batch by hand (the call pattern before this feature)."""
    from samplenet_amd import BatchRecipe, DeviceBatchSource, DeviceCloudSet
    from samplenet_amd.engine import SamplerTrainStep
    from samplenet_amd.parallel import FlatGradAllReducer
    from samplenet_amd.task_features import pcrnet_chamfer_loss

    pts, labels = _set()
    rc = BatchRecipe(shuffle_points=True, unit_cube=True)
    mk = lambda: DeviceBatchSource(DeviceCloudSet(pts, labels), rc, EB, EN, seed=6, pair="fixed")  # noqa: E731
    want = mk().at(0)
    pcr = _pcrnet(frozen=True, seed=1)
    task = lambda proj, p1: pcrnet_chamfer_loss(pcr, proj, p1)[0]  # noqa: E731
    for use_graph in (False, True):
        na, nb = _nets(2)
        ra, rb = FlatGradAllReducer(na), FlatGradAllReducer(nb)
        p1 = want.p1.clone()
        sa = SamplerTrainStep(na, want.p0, reducer=ra, task_loss=task, use_graph=use_graph, input_source=mk())
        sb = SamplerTrainStep(nb, want.p0, reducer=rb, task_loss=lambda proj: task(proj, p1), use_graph=use_graph)
        assert sa.igt is None and sb.igt is None
        la, lb = sa.step(), sb(want.p0)
        torch.cuda.synchronize()
        assert torch.equal(_bits(la), _bits(lb)) and torch.isfinite(la) and torch.equal(_bits(ra.flat), _bits(rb.flat)), use_graph
