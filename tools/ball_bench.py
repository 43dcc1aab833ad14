#!/usr/bin/env python3
"""The ball query and the fused query-and-group on the GPU (samplenet_amd/csrc/ball_query.hip): HIP-event timing of sn_ball_query at
the reference harness's shape (classification/grouping/test/query_ball_point.cpp:88-89) and of sn_ball_query, sn_ball_group_forward
and sn_ball_group_backward at two set-abstraction shapes, each beside the composition of torch ops a user would otherwise write, and
the fused pair also beside the composition of this library's own launches (sn_ball_query + sn_grouping_operation + a subtraction;
sn_grouping_operation_grad + sums back).  Reports whether the routes agree beside their timings.  Output: profiles/ball/ball_bench.txt.

    python tools/ball_bench.py
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from samplenet_amd import ops  # noqa: E402
from samplenet_amd._lib import check, lib, ptr  # noqa: E402

QUERY_SHAPES = [  # (b, n, m, radius, nsample, c, what it is)
    (32, 512, 128, 0.1, 64, 0, "the reference harness's shape"),
    (32, 1024, 512, 0.2, 32, 0, "set abstraction 1: 1024 -> 512, xyz only"),
    (32, 512, 128, 0.4, 64, 128, "set abstraction 2: 512 -> 128, 128 features"),
]


def timed(fn, target_s=0.5):
    """mean ms per call: 3 warm-up calls, then enough calls for ~target_s"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    reps = max(10, min(2000, int(target_s * 1e3 / max(e0.elapsed_time(e1), 1e-3))))
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def torch_ball_query(radius, nsample, xyz, new_xyz):
    """the usual torch formulation (squared rule): distances, mask, sort of the masked index grid, first-hit padding"""
    b, n, _ = xyz.shape
    m = new_xyz.shape[1]
    d2 = ((new_xyz[:, :, None, :] - xyz[:, None, :, :]) ** 2).sum(-1)
    grid = torch.arange(n, device=xyz.device).view(1, 1, n).expand(b, m, n).clone()
    r = torch.tensor(radius, dtype=torch.float32, device=xyz.device)
    grid[d2 >= r * r] = n
    idx = grid.sort(dim=-1).values[:, :, :nsample]
    first = idx[:, :, :1].expand(-1, -1, idx.shape[2])
    idx = torch.where(idx == n, first, idx)
    return torch.where(idx == n, torch.zeros_like(idx), idx)  # an empty ball: zeros, as the kernel writes


def torch_group(xyz, new_xyz, features, idx, use_xyz=True):
    b, m, ns = idx.shape
    li = idx.long().reshape(b, 1, m * ns)
    parts = []
    if use_xyz:
        parts.append(torch.gather(xyz.transpose(1, 2), 2, li.expand(b, 3, m * ns)).view(b, 3, m, ns) - new_xyz.transpose(1, 2).unsqueeze(-1))
    if features is not None:
        c = features.shape[1]
        parts.append(torch.gather(features, 2, li.expand(b, c, m * ns)).view(b, c, m, ns))
    return torch.cat(parts, 1)


def own_group(radius, nsample, xyz, new_xyz, features):
    """this library's own launches, composed: query, gather of the cloud as three channels, subtraction, gather of the features"""
    idx, _ = ops.ball_query(radius, nsample, xyz, new_xyz, rule="squared")
    parts = [ops.grouping_operation(xyz.transpose(1, 2).contiguous(), idx) - new_xyz.transpose(1, 2).unsqueeze(-1)]
    if features is not None:
        parts.append(ops.grouping_operation(features, idx))
    return torch.cat(parts, 1) if len(parts) > 1 else parts[0]


def main():
    assert torch.cuda.is_available(), "ball_bench.py measures on a GPU"
    torch.manual_seed(0)
    lines = ["# tools/ball_bench.py on %s; HIP events, mean ms per call over >= 10 calls after 3 warm-up calls; squared rule unless named"
             % torch.cuda.get_device_name(0),
             "# torch: distances + masked sort + gathers; own: sn_ball_query + sn_grouping_operation (+ subtraction, cat) of this library",
             "%-46s %10s %10s %10s" % ("shape (b, n -> m, r, nsample, c)", "fused ms", "own ms", "torch ms")]
    for b, n, m, r, ns, c, what in QUERY_SHAPES:
        xyz, new = torch.rand(b, n, 3, device="cuda"), torch.rand(b, m, 3, device="cuda")
        feat = torch.rand(b, c, n, device="cuda") if c else None
        tag = "(%d, %d -> %d, %g, %d, %d)" % (b, n, m, r, ns, c)
        lines.append("# " + what)
        # the query alone, both rules
        ref = torch_ball_query(r, ns, xyz, new)
        idx, cnt = ops.ball_query(r, ns, xyz, new, rule="squared")
        lines.append("#   rows that differ from the torch formulation: %d" % int((idx.long() != ref).any(-1).sum()))
        lines.append("#   mean hits per query %.1f of %d, empty balls %d of %d" % (float(cnt.float().mean()), ns, int((cnt == 0).sum()), b * m))
        t_sq = timed(lambda: ops.ball_query(r, ns, xyz, new, rule="squared"))
        t_rt = timed(lambda: ops.ball_query(r, ns, xyz, new, rule="sqrt"))
        t_torch = timed(lambda: torch_ball_query(r, ns, xyz, new))
        lines.append("%-46s %10.4f %10s %10.4f" % ("query   " + tag, t_sq, "-", t_torch))
        lines.append("%-46s %10.4f %10s %10s" % ("query, sqrt rule", t_rt, "-", "-"))
        if (b, n, m, r, ns, c) == QUERY_SHAPES[0][:6]:
            continue
        # forward
        fused = ops.ball_group(r, ns, xyz, new, feat)
        lines.append("#   fused == own composition: %s, == torch composition: %s"
                     % (torch.equal(fused, own_group(r, ns, xyz, new, feat)), torch.equal(fused, torch_group(xyz, new, feat, idx))))
        t_f = timed(lambda: ops.ball_group(r, ns, xyz, new, feat))
        t_o = timed(lambda: own_group(r, ns, xyz, new, feat))
        t_t = timed(lambda: torch_group(xyz, new, feat, torch_ball_query(r, ns, xyz, new)))
        lines.append("%-46s %10.4f %10.4f %10.4f" % ("forward " + tag, t_f, t_o, t_t))
        # backward (all three gradients), timed as forward + backward minus the forward above
        g = torch.rand_like(fused)
        leaves = [t.clone().requires_grad_(True) for t in ((xyz, new, feat) if c else (xyz, new))]

        def step(route):
            for t in leaves:
                t.grad = None
            f = leaves[2] if c else None
            if route == "fused":
                out = ops.ball_group(r, ns, leaves[0], leaves[1], f)
            elif route == "own":
                out = own_group(r, ns, leaves[0], leaves[1], f)
            else:
                out = torch_group(leaves[0], leaves[1], f, idx)
            out.backward(g)

        step("fused")
        gf = [t.grad.clone() for t in leaves]
        step("torch")
        lines.append("#   worst gradient difference from the torch formulation: %.3g"
                     % max(float((a - t.grad).abs().max()) for a, t in zip(gf, leaves)))
        t_fb, t_ob, t_tb = (timed(lambda route=route: step(route)) for route in ("fused", "own", "torch"))
        lines.append("%-46s %10.4f %10.4f %10.4f" % ("fwd+bwd " + tag, t_fb, t_ob, t_tb))
        lines.append("#   (torch's fwd+bwd reuses precomputed indices: its query is not in that row)")
        # the backward entry alone: all three gradients
        gx, gn = torch.empty(b, n, 3, device="cuda"), torch.empty(b, m, 3, device="cuda")
        gfe = torch.empty(b, c, n, device="cuda") if c else None
        st = torch.cuda.current_stream().cuda_stream
        t_b = timed(lambda: check(lib.sn_ball_group_backward(b, n, m, c, ns, 1, ptr(idx), ptr(g), ptr(gfe), ptr(gx), ptr(gn), st)))
        lines.append("%-46s %10.4f %10s %10s" % ("sn_ball_group_backward alone", t_b, "-", "-"))
    text = "\n".join(lines) + "\n"
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ball", "ball_bench.txt")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
