"""The references, generators and tables of tests/mlp_ref.py, on the CPU (no GPU, no library call): every reference against torch's
own fp64 BatchNorm1d / Linear / amax composition to 1e-12 relative, the generators' conditions under which tests/test_gpu_mlp_direct.py
may compare EVERY element (pool values distinct as fp32 numbers except for the planted ties; every ReLU argument of the layer backward
further from 0 than its rounding), the hand-evaluated loop tables against the loops, and the route predicates against the sources."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mlp_ref as M  # noqa: E402

CPU = torch.device("cpu")
TOL = 1e-12


def close(a, b, what):
    a, b = a.detach().double(), b.detach().double()
    scale = max(float(a.abs().max()), float(b.abs().max()), 1e-300)
    assert float((a - b).abs().max()) <= TOL * scale, (what, float((a - b).abs().max()), scale)


def _bn(C, c, train=True):
    bn = torch.nn.BatchNorm1d(C, eps=M.EPS, momentum=M.MOMENTUM).double()
    with torch.no_grad():
        bn.weight.copy_(c.gamma.double()), bn.bias.copy_(c.beta.double())
        bn.running_mean.copy_(c.rm.double()), bn.running_var.copy_(c.rv.double())
        bn.num_batches_tracked.fill_(7)
    return bn.train(train)


@pytest.mark.parametrize("R,C", [(33, 5), (129, 36), (300, 64)])
def test_training_batchnorm_against_torch(R, C):
    """twopass_ref (from z) and finalize_ref (from block sums of the same z, kept in fp64) give torch.nn.BatchNorm1d(double)'s output,
    running statistics and counter."""
    c = M.twopass_case(R, C, CPU)
    bn = _bn(C, c)
    y = bn(c.z.double())
    nblk = (R + 63) // 64
    blocks = [c.z.double()[b * 64:(b + 1) * 64] for b in range(nblk)]
    f = M.Case(nblk=nblk, C=C, R=R, stats=torch.stack([torch.stack([b.sum(0), (b * b).sum(0)]) for b in blocks]), gamma=c.gamma, beta=c.beta,
               rm=c.rm, rv=c.rv)
    for name, ref in (("twopass", M.twopass_ref(c)), ("finalize", M.finalize_ref(f))):
        live = torch.arange(C) != 3 if name == "finalize" else slice(None)  # (the constant channel: ss / R - mean^2 is rounding noise times 1e5)
        close((c.z.double() * ref["scale"][0] + ref["shift"][0])[:, live], y[:, live], (name, "y"))
        close(ref["running_mean"][0], bn.running_mean, (name, "running_mean"))
        close(ref["running_var"][0][live], bn.running_var[live], (name, "running_var"))
        close(ref["mean"][0], c.z.double().mean(0), (name, "mean"))
        close(ref["invstd"][0][live], ((c.z.double().var(0, unbiased=False) + M.EPS) ** -0.5)[live], (name, "invstd"))
        for v, e in ref.values():
            assert bool((e >= 0).all()) and bool(torch.isfinite(e).all()) and bool(torch.isfinite(v).all())
    assert int(bn.num_batches_tracked) == 8  # the entries add 1 to the counter they are given: asserted on the GPU
    bare = M.twopass_ref(c, with_running=False)
    assert "running_mean" not in bare and "running_var" not in bare  # running_mean == NULL: both stay untouched


def test_one_row_keeps_the_biased_variance():
    """THE CONTRACT for R == 1 (torch refuses it in training mode): bn_finalize_channel_mv's `R > 1 ? var R / (R - 1) : var`."""
    c = M.finalize_case(1, 8, 1, CPU)
    ref = M.finalize_ref(c)
    st = c.stats.double()
    var = (st[0, 1] - st[0, 0] ** 2).clamp_min(0)
    close(ref["running_var"][0], (1 - M.MOMENTUM) * c.rv.double() + M.MOMENTUM * var, "running_var at R = 1")
    close(ref["mean"][0], st[0, 0], "mean at R = 1")


def test_constant_channel_and_conditioning():
    """Every finalize / twopass case carries |mean| / std = 0, 3, 100 on channels 0..2 and a constant channel 3 whose invstd is
    1 / sqrt(eps); the bounds of all four stay at a few U (no conditioning factor)."""
    for nblk, R in M.ROWS_OF_NBLK.items():
        c = M.finalize_case(nblk, 8, R, CPU)
        ref = M.finalize_ref(c)
        st = c.stats.double().sum(0) / R
        ratio = st[0].abs() / (st[1] - st[0] ** 2).clamp_min(1e-300).sqrt()
        assert float(ratio[0]) < 0.2 and 2.5 < float(ratio[1]) < 3.5 and 80 < float(ratio[2]) < 125, (nblk, ratio[:3])
        assert abs(float(ref["invstd"][0][3]) * M.EPS ** 0.5 - 1) < 1e-9
        for name in ("invstd", "scale", "mean"):
            v, e = ref[name]
            # (the constant channel at 1000 blocks: 1004 D on ss / R = 4 against eps = 1e-5 is 0.75 U of invstd, the largest double term here)
            assert bool((e[:4] <= 4 * M.U * v.abs()[:4] + 1e-300).all()), (nblk, name)
    for R in M.TWOPASS_TABLE:
        c = M.twopass_case(R, 8, CPU)
        ref = M.twopass_ref(c)
        zd = c.z.double()
        ratio = zd.mean(0).abs() / zd.std(0, unbiased=False).clamp_min(1e-300)
        assert float(ratio[0]) < 1e-6 and abs(float(ratio[1]) - 3) < 1e-3 and abs(float(ratio[2]) - 100) < 1e-1 and float(zd[:, 3].std()) == 0
        v, e = ref["invstd"]
        assert bool((e <= 1.01 * M.U * v).all()), R


@pytest.mark.parametrize("C", [5, 64])
def test_eval_batchnorm_against_torch(C):
    c = M.eval_case(C, CPU)
    ref = M.eval_coef_ref(c)
    z = torch.randn(9, C, dtype=torch.float64, generator=torch.Generator().manual_seed(C))
    close(z * ref["scale"][0] + ref["shift"][0], _bn(C, c, train=False)(z), "eval y")
    close(ref["mean"][0], c.rm, "eval mean")


def _coef64(z, gamma, beta, mean=None, var=None):
    mean = z.mean(0) if mean is None else mean
    var = z.var(0, unbiased=False) if var is None else var
    inv = (var + M.EPS) ** -0.5
    return torch.stack([gamma * inv, beta - mean * gamma * inv, mean, inv])


@pytest.mark.parametrize("train", [True, False])
def test_batchnorm_backward_against_autograd(train):
    """dZ = k1 dY + k2 Z + k3, dgamma, dbeta against torch.autograd.grad through BatchNorm1d(double); eval mode = the `fixed` form
    (k2 = k3 = 0, dgamma / dbeta of the same form); dbias = sum_r dZ."""
    R, C = 37, 9
    g = M.gen(11, CPU)
    c = M.Case(gamma=M.randn(g, C), beta=M.randn(g, C), rm=M.randn(g, C), rv=M.rand(g, C) + 0.5)
    z = (M.randn(g, R, C).double() * 1.5 + 0.5).requires_grad_()
    dy = M.randn(g, R, C).double()
    bn = _bn(C, c, train)
    dz, dgamma, dbeta = torch.autograd.grad(bn(z), (z, bn.weight, bn.bias), dy)
    zd = z.detach()
    coef = _coef64(zd, c.gamma.double(), c.beta.double()) if train else _coef64(zd, c.gamma.double(), c.beta.double(), c.rm.double(), c.rv.double())
    s, dg = dy.sum(0), coef[3] * (dy * (zd - coef[2])).sum(0)
    zero = torch.zeros_like(s)
    ref = M.bn_backward_ref(coef, dg, zero, s, zero, R, fixed=not train)
    k = ref["kcoef"][0]
    close(k[0] * dy + k[1] * zd + k[2], dz, "dZ")
    close(ref["dgamma"][0], dgamma, "dgamma"), close(ref["dbeta"][0], dbeta, "dbeta")
    assert float((ref["dbias"][0] - dz.sum(0)).abs().max()) <= TOL * float(dy.abs().sum(0).max()), "dbias = sum_r dZ"
    if not train:
        assert not bool(k[1:].any())
        close(ref["dbias"][0], coef[0] * s, "dbias on fixed statistics = k1 s")


def test_batchnorm_under_the_max_pool_against_autograd():
    """prev_bn_rows > 0: BatchNorm over B N rows -> ReLU -> max over the points, only B rows per channel carry a gradient.  From
    pool_forward_ref's pick and pool_backward_ref's sums: dZ (B N, C) = k1 dY + k2 Z + k3 with dY = gsel scattered to argsel, against
    autograd through torch's composition; dbias = sum_r dZ."""
    B, N, C = 4, 12, 10
    g = M.gen(12, CPU)
    gamma, beta = M.randn(g, C).double(), M.randn(g, C).double() * 0.5
    gamma[0], gamma[1] = -1.0, 1.0
    x = M.randn(g, B, N, C).double().requires_grad_()
    up = M.randn(g, B, C).double()
    bn = torch.nn.BatchNorm1d(C, eps=M.EPS).double().train()
    with torch.no_grad():
        bn.weight.copy_(gamma), bn.bias.copy_(beta)
    pooled = torch.relu(bn(x.view(B * N, C))).view(B, N, C).amax(1)
    dz, dgamma, dbeta = torch.autograd.grad(pooled, (x, bn.weight, bn.bias), up)
    xd = x.detach()
    coef = _coef64(xd.view(B * N, C), gamma, beta)
    arg, zsel, pooled_ref, _ = M.pool_forward_ref(xd, coef)
    close(pooled_ref, pooled, "pooled")
    assert bool((gamma < 0).any()) and bool((pooled_ref == 0).any()) and bool((pooled_ref > 0).any())
    c = M.Case(B=B, C=C, g=up, pooled=pooled_ref, zsel=zsel, coef=coef)
    ref = M.pool_backward_ref(c, rows=B * N)
    dy = torch.zeros(B, N, C, dtype=torch.float64).scatter_(1, arg.long()[:, None, :], ref["gsel"][0][:, None, :])
    k = ref["kcoef"][0]
    close(k[0] * dy + k[1] * xd + k[2], dz, "dZ under the pool")
    close(ref["dgamma"][0], dgamma, "dgamma"), close(ref["dbeta"][0], dbeta, "dbeta")
    assert float((ref["dbias"][0] - dz.sum((0, 1))).abs().max()) <= TOL * float(up.abs().sum(0).max())
    fixed = M.pool_backward_ref(c, fixed=True)
    assert not bool(fixed["kcoef"][0][1:].any())
    close(fixed["dgamma"][0], ref["dgamma"][0], "dgamma unchanged on fixed statistics"), close(fixed["dbeta"][0], ref["dbeta"][0], "dbeta")


_ALL_BWD = [(s, M.SMALL_BWD_FORMS) for s, _ in M.SMALL_BWD_TABLE] + [(s, M.LAYER_BWD_FORMS) for (s, _db), _ in M.LAYER_BWD_TABLE]


@pytest.mark.parametrize("shape,forms", _ALL_BWD, ids=["R%d-Ci%d-Co%d-dz%d-npts%d" % s for s, _ in _ALL_BWD])
def test_layer_backward_against_autograd(shape, forms):
    """layer_backward_ref in the three dz_modes and the three forms against autograd through Linear(act(zprev)) with the BatchNorm of the
    layer below written out (batch statistics over the R rows; averaged over 64 R rows of which R are here; fixed)."""
    R, Ci, Co, mode, npts = shape
    for form in forms:
        c = M.layer_backward_case(shape, form, CPU)
        ref = M.layer_backward_ref(c, M.layer_backward_route(R, Ci, Co, mode, npts, False))
        small = M.layer_backward_ref(c)  # the centred and the partial-sum forms of dgamma are the same number
        close(ref["prev_dgamma"][0], small["prev_dgamma"][0], (form, "dgamma, both forms"))
        dz, _e = M.dz_ref(c)
        zp = c.zprev.double().requires_grad_()
        W = c.W.double().requires_grad_()
        sc, sh = c.coef_prev[0].double(), c.coef_prev[1].double()
        a = torch.relu(zp * sc + sh)
        dyprev, dW = torch.autograd.grad(torch.nn.functional.linear(a, W), (a, W), dz)
        close(ref["dW"][0], dW, (form, "dW")), close(ref["db"][0], dz.sum(0), (form, "db"))
        live = (zp.detach() * sc + sh > 0).double()
        close(ref["dyprev"][0], dyprev * live, (form, "dyprev"))
        gv, mean, inv = dyprev * live, c.coef_prev[2].double(), c.coef_prev[3].double()
        close(ref["prev_dbeta"][0], gv.sum(0), (form, "dbeta")), close(ref["prev_dgamma"][0], inv * (gv * (zp.detach() - mean)).sum(0), (form, "dgamma"))
        k = ref["prev_kcoef"][0]
        if form == "fixed":
            assert not bool(k[1:].any())
        if form == "rows":  # autograd through the normalisation itself (gamma = scale / invstd as the forward had it)
            zq = c.zprev.double().requires_grad_()
            m, v = zq.mean(0), zq.var(0, unbiased=False)
            xhat = (zq - m) * (v + M.EPS) ** -0.5
            want, = torch.autograd.grad(xhat * (sc / inv), zq, gv)
            got = k[0] * gv + k[1] * c.zprev.double() + k[2]
            # coef_prev holds the fp32 roundings of mean / invstd: the two agree to that rounding, not to 1e-12
            assert float((got - want).abs().max()) <= 64 * M.U * float(gv.abs().max() * sc.abs().max()), (form, "dZprev")
            assert float(ref["prev_dbias"][0].abs().max()) <= 1e-12 * R * float((k[1] * mean).abs().max() + k[2].abs().max() + 1), "dbias = 0"
        assert M.relu_margin(c) < 1.0, (shape, form, M.relu_margin(c))
        pre = c.zprev.double() * sc + sh
        assert bool((pre[:, 4] == 0).all()) and bool((ref["dyprev"][0][:, 4] == 0).all())  # the exact zeros: masked by `> 0`
        assert float((dz @ c.W.double())[:, 4].abs().min()) > 0                              # ... with a gradient above them


def test_pool_generator_conditions():
    """For every row of the pool tables: along the points all values differ as fp32 numbers except the planted pairs, each planted
    pair is bit-identical and IS the value its channel selects; scales of both signs, one +0.0 and one -0.0; every arrangement of
    ties occurs in the table, and the first row wins in the reference."""
    seen = set()
    for N in M.POOL_FWD_TABLE:
        for C in M.POOL_FWD_C:
            c = M.pool_case(N, C, CPU)
            sc = c.coef[0]
            assert bool((sc > 0).any()) and bool((sc < 0).any()) and float(sc[2]) == 0 and float(sc[3]) == 0
            assert not bool(torch.signbit(sc[2])) and bool(torch.signbit(sc[3]))
            planted = torch.zeros(c.B, N, C, dtype=torch.bool)
            arg, zsel, pooled, _ = M.pool_forward_ref(c.z, c.coef)
            for name, b, n0, n1, ch in c.ties:
                seen.add(name)
                planted[b, n1, ch] = True
                assert c.z[b, n0, ch].view(torch.int32) == c.z[b, n1, ch].view(torch.int32) and n0 < n1
                assert int(arg[b, ch]) == n0 and float(zsel[b, ch]) == float(c.z[b, n0, ch]), (N, C, name)
            srt = torch.where(planted, torch.full_like(c.z, float("inf")), c.z).sort(1).values
            gaps = srt[:, 1:] - srt[:, :-1]
            assert bool((gaps[torch.isfinite(gaps)] > 0).all()), (N, C)
            assert bool((pooled == 0).any()) and bool((pooled > 0).any())
    assert seen == {name for name, _ in M.TIE_ARRANGEMENTS}
    for B in M.POOL_BWD_TABLE:
        for recipe in ("real",) + (("integer",) if B & (B - 1) == 0 else ()):
            c = M.pool_backward_case(recipe, B, 40, CPU)
            dead = c.pooled == 0
            assert bool(dead.any()) and bool((c.g[dead] != 0).all()) and bool((c.pooled >= 0).all()), B


def test_integer_recipes_are_exact():
    """The integer recipes' references are fp32 numbers (so `bit for bit` is a fair demand whatever the summation order: every partial
    sum is an integer multiple of the unit below 2^24 of it)."""
    exact = lambda t: bool((t.float().double() == t).all())
    for nblk in M.PARTIAL_SUMS_TABLE:
        for C in M.PARTIAL_SUMS_C:
            c = M.backward_coef_case("integer", nblk, C, M.int_rows(nblk), CPU)
            for name, (v, e) in M.backward_coef_ref(c).items():
                assert exact(v), (nblk, C, name)
    for B in (b for b in M.POOL_BWD_TABLE if b & (b - 1) == 0):
        for C in M.POOL_BWD_C:
            c = M.pool_backward_case("integer", B, C, CPU)
            for ref in (M.pool_backward_ref(c, rows=B * M.POOL_BWD_N), M.pool_backward_ref(c, fixed=True)):
                for name, (v, e) in ref.items():
                    assert exact(v.double()), (B, C, name)


def test_tables_against_the_loops():
    """Each row's hand-evaluated trip counts are what the loops give; no two rows of a table reach the same branch."""
    for name, (table, lanes, unroll) in M.LOOPS.items():
        keys = set()
        for size, (branch, first, last) in table.items():
            assert M.trips(size, 0, lanes, unroll) == first and M.trips(size, lanes - 1, lanes, unroll) == last, (name, size, branch)
            keys.add((first, last, min(size, lanes)))
        assert len(keys) == len(table), name
        assert any(f[0] == 0 and l[0] == 0 for _, f, l in table.values()) and any(f[0] > 0 and l[0] == 0 for _, f, l in table.values())
        assert any(l[0] > 0 for _, f, l in table.values()), name
    k = M.source_constants()
    assert k == {"TileBig::BM": 64, "TileSmall::BM": 32}
    assert set(M.ROWS_OF_NBLK) == set(M.PARTIAL_SUMS_TABLE)
    for nblk, R in M.ROWS_OF_NBLK.items():
        assert M.stats_blocks(R, k) == nblk, (nblk, R)
    assert [M.stats_blocks(R, k) for R in (1, 32, 33, 64, 65, 128, 129)] == [1, 1, 2, 2, 2, 2, 3]
    shapes = [s for s, _ in M.SMALL_BWD_TABLE]
    assert {s[3] for s in shapes} == {0, 1, 2} and all(s[0] <= 32 for s in shapes)
    assert {(s[3], s[2] % 64 == 0) for s in shapes} == {(m, v) for m in (0, 1, 2) for v in (True, False)}  # every dz_mode on both load paths
    assert all(s[0] % s[4] == 0 for s in shapes if s[3] == 2)


def test_every_route_of_the_layer_backward_has_its_rows():
    """Each row of LAYER_BWD_TABLE reaches the route it names (the dispatch restated predicate by predicate), the five routes are all
    there, each in every dz_mode it serves, and the split count restated equals the table's use of it."""
    served = {"fused": {1, 2}, "rows<=64": {0, 1}, "rows>64": {0, 1}, "fast": {0, 1, 2}, "fallback": {0, 1, 2}}
    seen = {}
    for (shape, db), (route, why) in M.LAYER_BWD_TABLE:
        assert M.layer_backward_route(*shape, db) == route, (shape, db, why)
        seen.setdefault(route, set()).add(shape[3])
        assert shape[0] > 32 and (shape[3] != 2 or shape[0] % shape[4] == 0)
    assert seen == served, seen
    assert {(s[1], s[2]) for (s, _), (r, _w) in M.LAYER_BWD_TABLE if r == "fused"} == set(M.FUSED_SHAPES)
    assert len({k for k, _ in M.LAYER_BWD_TABLE}) == len(M.LAYER_BWD_TABLE)
    for (shape, _db), _ in M.LAYER_BWD_TABLE:  # a fused workgroup's partial covers at most 64 rows (STATS_SCHEME's count)
        R, Ci, Co = shape[:3]
        tr = 32 if (Ci, Co) in ((128, 128), (128, 256), (256, 128)) else 64
        tiles, groups = -(-R // tr), -(-R // 64)
        assert -(-tiles // groups) * tr <= 64, shape
    for shape in M.ALONE_TABLE:
        assert M.layer_backward_route(*shape, False) in ("small", "fast")


def test_every_route_of_the_layer_forward_has_its_rows():
    """LAYER_FWD_TABLE against the dispatch restated; every route there, with and without coef_prev and running statistics somewhere;
    layer_z_ref is torch's Linear on the activation; layer_stats_ref of that z is BatchNorm1d's training-mode update."""
    seen = set()
    for (shape, prev, running), (route, why) in M.LAYER_FWD_TABLE:
        assert M.layer_forward_route(*shape, prev) == route, (shape, why)
        seen.add(route)
        c = M.layer_forward_case(shape, prev, CPU)
        z, e = M.layer_z_ref(c)
        a = c.ain.double() if not prev else torch.relu(c.ain.double() * c.coef_prev[0].double() + c.coef_prev[1].double())
        close(z, torch.nn.functional.linear(a, c.W.double(), c.bias.double()), (shape, "z"))
        bn = _bn(c.Co, c)
        y = bn(z)
        ref = M.layer_stats_ref(z, c, route)
        close(z * ref["scale"][0] + ref["shift"][0], y, (shape, "y"))
        close(ref["running_var"][0], bn.running_var, (shape, "running_var")), close(ref["running_mean"][0], bn.running_mean, (shape, "running_mean"))
    assert seen == set(M.FWD_STATS_SCHEME)
    assert {p for (_, p, _r), _ in M.LAYER_FWD_TABLE} == {True, False} == {r for (_, _p, r), _ in M.LAYER_FWD_TABLE}
    for (R, npts, Ci, Co), _ in M.CONV_POOL_TABLE:
        assert R > 64 and R % 64 == 0 and npts % 64 == 0 and R % npts == 0 and Ci % 64 == 0 and Co % 64 == 0
    assert any(npts > 64 for (_, npts, _, _), _ in M.CONV_POOL_TABLE)


def test_in3_closed_form_and_conv_stack_tables():
    """in3_ref's dW_in is the xyz layer's weight gradient dZprev^T x with dZprev = k1 dYprev + k2 zprev + k3, when zprev IS x W_in^T + b_in
    (in fp64: the closed form is an identity); in3_stats_floats and the conv-stack predicates on every table row."""
    c = M.in3_case(300, CPU)
    c.zprev = c.x.double() @ c.W_in.double().t() + c.b_in.double()  # exact: the identity holds to fp64 rounding
    assert M.relu_margin(c) < 1.0
    ref = M.in3_ref(c, 5)
    full = M.layer_backward_ref(c, "fused", 5)
    k, gv = ref["prev_kcoef"][0], full["dyprev"][0]
    dzprev = k[0] * gv + k[1] * c.zprev + k[2]
    close(ref["dW_in"][0], dzprev.t() @ c.x.double(), "dW_in closed form")
    assert bool((ref["dW_in"][1] >= 0).all()) and "dyprev" not in ref and "db" not in ref
    assert [(M.in3_stats_floats(*s) > 0) for s, _ok, _ in M.IN3_TABLE] == [ok for _, ok, _ in M.IN3_TABLE]
    assert M.in3_stats_floats(300, 64, 64) == 5 * 6 * 64 and sum(ok for _, ok, _ in M.IN3_TABLE) == 1
    for ((B, N), ch), (z1free, why) in M.CONV_STACK_TABLE:
        assert M.conv_stack_supported(B, N, ch) == 1 and M.conv_stack_z1_free(B, N, ch) == int(z1free), why
    assert ((2, 64), True) in [(bn, True) for (bn, _), _ in M.CONV_STACK_TABLE] and any(z for _, (z, _w) in M.CONV_STACK_TABLE)
    assert M.conv_stack_supported(1, 64, (3, 64, 128)) == 0 and M.conv_stack_supported(2, 96, (3, 64, 128)) == 0
    # conv_fx_stats_ref of an fp64 z is BatchNorm1d's update
    cs = M.conv_stack_case(2, 64, (3, 64, 128), CPU)
    lc = M.conv_stack_layer(cs, 0, None, None)
    z, _e = M.layer_z_ref(lc)
    bn = _bn(64, lc)
    y = bn(z)
    ref = M.conv_fx_stats_ref(z, lc)
    close(z * ref["scale"][0] + ref["shift"][0], y, "stack layer y"), close(ref["running_var"][0], bn.running_var, "stack running_var")


def test_route_predicates_in_the_sources():
    """The loops and predicates the tables were evaluated from still stand in the sources as read (an edit of one shows up here)."""
    found = M.source_routes()
    for name in M.ROUTE_PATTERNS:
        assert found[name] == M.ROUTE_COUNTS.get(name, 1), (name, found[name])
