#!/usr/bin/env python3
"""The set-abstraction level on the GPU (samplenet_amd/csrc/set_abstraction.hip, samplenet_amd/set_abstraction.py, the pointnet2
stand-in's PointnetSAModule): HIP-event timing through the Python surface at the three levels of a PointNet++ single-scale
classifier (as recalled), the columns of a row ALTERNATED inside one run -- every call times each column once, in turn --, at least
10 calls each, median and spread (min .. max) printed.

    module          forward and forward + backward, fused against fused=False (QueryAndGroup, torch Conv2d / BatchNorm2d / max_pool2d)
    grouping        ops.ball_group_rows against ops.ball_group + permute, forward and forward + backward
    pool            sn_group_pool_forward + sn_group_pool_backward + sn_bn_backward_coef against sn_pool_forward + sn_pool_backward_bn

Output: profiles/sa/sa_bench.txt (--out PATH to write elsewhere).

    python tools/sa_bench.py [--calls 12] [--out PATH]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from samplenet_amd import ops  # noqa: E402
from samplenet_amd._lib import check, lib, ptr  # noqa: E402
from samplenet_amd.compat.pointnet2.utils import pointnet2_modules as PM  # noqa: E402

B = 32
LEVELS = [  # (N, npoint, radius, nsample, C, mlp)
    (1024, 512, 0.2, 32, 0, [0, 64, 64, 128]),
    (512, 128, 0.4, 64, 128, [128, 128, 128, 256]),
    (128, None, None, None, 256, [256, 256, 512, 1024]),
]
POOL_SHAPES = [(16384, 32, 128), (4096, 64, 256), (32, 128, 1024), (32, 1024, 1024)]  # (G, S, C): C = the level's last width


def alternated(columns, calls):
    """columns: name -> fn.  Every call times each column once (`inner` launches between two events, about 5 ms), in turn.
    -> name -> (median ms, min ms, max ms) per launch"""
    inner = {}
    for name, fn in columns.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        inner[name] = max(1, min(200, int(5.0 / max(e0.elapsed_time(e1), 1e-3))))
    times = {name: [] for name in columns}
    for _ in range(calls):
        for name, fn in columns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner[name]):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / inner[name])
    return {name: (statistics.median(t), min(t), max(t)) for name, t in times.items()}


def fmt(res, order):
    return "  ".join("%s %8.4f (%.4f .. %.4f)" % ((n,) + res[n]) for n in order)


def ratio_line(res, new, old):
    """old / new of the medians, and whether the gap exceeds the larger spread"""
    gap = abs(res[old][0] - res[new][0])
    spread = max(res[new][2] - res[new][1], res[old][2] - res[old][1])
    return "#   %s / %s = %.2fx; |gap| %.4f ms, larger spread %.4f ms: %s" % (
        old, new, res[old][0] / res[new][0], gap, spread, "beyond the spread" if gap > spread else "WITHIN the spread")


def module_rows(lines, calls):
    for N, npoint, r, ns, C, mlp in LEVELS:
        torch.manual_seed(0)
        m = PM.PointnetSAModule(list(mlp), npoint=npoint, radius=r, nsample=ns).cuda().train()
        xyz = torch.rand(B, N, 3, device="cuda")
        f = torch.randn(B, C, N, device="cuda", requires_grad=True) if C else None
        tag = "%d x %d -> %s, r %s, nsample %s, mlp %s" % (B, N, npoint, r, ns, [mlp[0] + 3] + mlp[1:])
        with torch.no_grad():
            a, b_ = m(xyz, f)[1], m(xyz, f, fused=False)[1]
        lines.append("# " + tag)
        lines.append("#   fused against fused=False, forward values: worst difference %.3g (of %.3g)" % (float((a - b_).abs().max()), float(b_.abs().max())))

        def fwd(fused):
            with torch.no_grad():
                m(xyz, f, fused=fused)

        def step(fused):
            m.zero_grad(set_to_none=True)
            if f is not None:
                f.grad = None
            m(xyz, f, fused=fused)[1].sum().backward()

        res = alternated({"fused": lambda: fwd(True), "torch": lambda: fwd(False)}, calls)
        lines.append("module forward   ms  " + fmt(res, ("fused", "torch")))
        lines.append(ratio_line(res, "fused", "torch"))
        res = alternated({"fused": lambda: step(True), "torch": lambda: step(False)}, calls)
        lines.append("module fwd+bwd   ms  " + fmt(res, ("fused", "torch")))
        lines.append(ratio_line(res, "fused", "torch"))


def grouping_rows(lines, calls):
    for N, npoint, r, ns, C, _ in LEVELS[:2]:
        xyz = torch.rand(B, N, 3, device="cuda")
        new = xyz[:, :npoint].contiguous()
        rows_f = torch.randn(B, N, C, device="cuda", requires_grad=True) if C else None
        cm_f = rows_f.detach().transpose(1, 2).contiguous().requires_grad_(True) if C else None
        lines.append("# grouping %d x %d -> %d, r %g, nsample %d, c %d" % (B, N, npoint, r, ns, C))
        a = ops.ball_group_rows(r, ns, xyz, new, rows_f)
        b_ = ops.ball_group(r, ns, xyz, new, cm_f).permute(0, 2, 3, 1).contiguous()
        lines.append("#   rows == ball_group permuted: %s" % torch.equal(a, b_))
        g = torch.randn_like(a)
        xr = xyz.clone().requires_grad_(True)

        def rows_fwd():
            with torch.no_grad():
                ops.ball_group_rows(r, ns, xyz, new, rows_f)

        def perm_fwd():
            with torch.no_grad():
                ops.ball_group(r, ns, xyz, new, cm_f).permute(0, 2, 3, 1).contiguous()

        def rows_step():
            xr.grad = None
            if C:
                rows_f.grad = None
            ops.ball_group_rows(r, ns, xr, new, rows_f).backward(g)

        def perm_step():
            xr.grad = None
            if C:
                cm_f.grad = None
            ops.ball_group(r, ns, xr, new, cm_f).permute(0, 2, 3, 1).contiguous().backward(g)

        res = alternated({"rows": rows_fwd, "permute": perm_fwd}, calls)
        lines.append("grouping forward ms  " + fmt(res, ("rows", "permute")))
        lines.append(ratio_line(res, "rows", "permute"))
        res = alternated({"rows": rows_step, "permute": perm_step}, calls)
        lines.append("grouping fwd+bwd ms  " + fmt(res, ("rows", "permute")))
        lines.append(ratio_line(res, "rows", "permute"))


def pool_rows(lines, calls):
    st = torch.cuda.current_stream().cuda_stream
    for G, S, C in POOL_SHAPES:
        z = torch.randn(G * S, C, device="cuda")
        coef = torch.stack([torch.randn(C), torch.randn(C) * 0.3, torch.randn(C) * 0.1, torch.rand(C) + 0.5]).cuda().contiguous()
        g = torch.randn(G, C, device="cuda")
        pooled, argsel, zsel, gsel = (torch.empty(G, C, device="cuda"), torch.empty(G, C, device="cuda", dtype=torch.int32),
                                      torch.empty(G, C, device="cuda"), torch.empty(G, C, device="cuda"))
        nblk = lib.sn_group_pool_stats_blocks(G)
        stats = torch.empty(nblk, 2, C, device="cuda")
        dg, db, dbias, kc = [torch.empty(C, device="cuda") for _ in range(3)] + [torch.empty(3, C, device="cuda")]

        def new_fwd():
            check(lib.sn_group_pool_forward(G, S, C, ptr(z), ptr(coef), ptr(pooled), ptr(argsel), ptr(zsel), st))

        def old_fwd():
            check(lib.sn_pool_forward(G, S, C, ptr(z), ptr(coef), ptr(pooled), ptr(argsel), ptr(zsel), st))

        def new_bwd():
            check(lib.sn_group_pool_backward(G, C, ptr(g), ptr(pooled), ptr(zsel), ptr(gsel), ptr(stats), st))
            check(lib.sn_bn_backward_coef(nblk, C, G * S, ptr(stats), ptr(coef), ptr(dg), ptr(db), ptr(dbias), ptr(kc), st))

        def old_bwd():
            check(lib.sn_pool_backward_bn(G, C, G * S, ptr(g), ptr(pooled), ptr(zsel), ptr(gsel), ptr(coef), ptr(dg), ptr(db), ptr(dbias),
                                          ptr(kc), st))

        lines.append("# pool (G, S, C) = (%d, %d, %d)" % (G, S, C))
        res = alternated({"group": new_fwd, "existing": old_fwd}, calls)
        lines.append("pool forward     ms  " + fmt(res, ("group", "existing")))
        lines.append(ratio_line(res, "group", "existing"))
        res = alternated({"group": new_bwd, "existing": old_bwd}, calls)
        lines.append("pool backward    ms  " + fmt(res, ("group", "existing")))
        lines.append(ratio_line(res, "group", "existing"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sa", "sa_bench.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available() and args.calls >= 10, "sa_bench.py measures on a GPU, at least 10 calls per column"
    lines = ["# tools/sa_bench.py on %s; HIP events; per column: median ms (min .. max) over %d calls, the columns of a row alternated"
             % (torch.cuda.get_device_name(0), args.calls)]
    pool_rows(lines, args.calls)
    grouping_rows(lines, args.calls)
    module_rows(lines, args.calls)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
