"""The registration task network's extractor entries called directly, table row by table row (tests/task_net_ref.py), against fp64:
sn_linear_forward_maxpool, sn_linear_forward_maxpool_wide, sn_pool_dgrad_sparse, sn_pointnet_narrow_forward and
sn_pointnet_narrow_backward.

Until now these were reached only through PointNetFeatures (tests/test_gpu_mlp.py), mostly one HIP route against another -- routes
that share gemm_tile_bx3, split3, pool_key, the decode kernels and the host glue --, on torch.rand inputs (no tie ever), always with
a bias and identity tables.  Here every output and scratch is a view into a sentinel-filled buffer of exactly the documented size
(check(): nothing outside it changed), EVERY element is compared -- integer data bit for bit, real data under bounds counted from the
kernels' operations, picks and masks exactly (tests/test_task_net_host.py proves the generators' conditions) -- duplicate rows are
planted at every distance at which another piece of the first-row-on-ties logic decides, and every case runs twice and must repeat
bit for bit.  Run with -s for the figures of profiles/task_net/errors.txt."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import task_net_ref as T  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
RECIPES = ("integer", "real")


def under(got, ref, bound, what):
    """element by element |got - ref| <= bound; -> worst err / bound (0 where both are 0)"""
    err = (got.double() - ref).abs()
    ok = err <= bound
    assert bool(ok.all()), (what, "worst err / bound", float((err / bound.clamp_min(1e-300))[~ok].max()), "at", int((~ok).flatten().nonzero()[0]))
    return float((err / bound.clamp_min(1e-300))[err > 0].max()) if bool((err > 0).any()) else 0.0


def held(got, ref, bound, exact, what):
    """integer recipes: bit for bit (-> 0); real ones: under the bound (-> worst ratio)"""
    if exact:
        assert torch.equal(got.double(), ref), (what, "bit for bit", int((got.double() != ref).sum()))
        return 0.0
    return under(got, ref, bound, what)


def note(worst, name, value):
    worst[name] = max(worst.get(name, 0.0), value)


def report(entry, key, worst):
    if worst:
        print("\ntask_net %s %s: worst err / bound  %s" % (entry, key, "  ".join("%s %.3f" % kv for kv in sorted(worst.items()))))


def same_bits(a, b, what):
    assert set(a) == set(b), (what, sorted(a), sorted(b))
    for name in a:
        assert torch.equal(a[name].view(torch.int32), b[name].view(torch.int32)), (what, "not the same bits", name)


def _bits(t):
    return t.view(torch.int32)


# ---- the two pooled entries ----------------------------------------------------------------------------------------------------------
def check_storing(call, c, ref, exact, worst):
    """A call that stores z, held to its own z: argsel the FIRST argmax of the stored z per cloud and column, zsel = z[argsel],
    pooled = relu of that, all exactly; z and pooled against fp64; the planted duplicate rows: the same bits, the maximum of some
    columns, and the lower row picked there."""
    z64, bnd, p64, pbnd = ref
    for t in (call.z, call.pooled, call.argsel, call.zsel):
        assert call.filled(t), call.what
    note(worst, "z", held(call.z, z64, bnd, exact, (call.what, "z")))
    m, first = T.first_argmax(call.z, c.B, c.npts)
    assert torch.equal(call.argsel, first), (call.what, "argsel is not the first argmax of z", (call.argsel != first).nonzero()[:4].tolist())
    assert torch.equal(_bits(call.zsel), _bits(m)), (call.what, "zsel")
    assert torch.equal(_bits(call.zsel), _bits(torch.gather(call.z.view(c.B, c.npts, c.Co), 1, call.argsel.long()[:, None, :])[:, 0])), (call.what, "zsel = z[argsel]")
    assert torch.equal(_bits(call.pooled), _bits(torch.where(m < 0, torch.zeros_like(m), m))), (call.what, "pooled = relu(zsel)")
    note(worst, "pooled", held(call.pooled, p64, pbnd, exact, (call.what, "pooled")))
    zc = call.z.view(c.B, c.npts, c.Co)
    if c.ties:
        tb, tp, td = (torch.tensor(col, device=DEV) for col in zip(*c.ties))
        assert torch.equal(_bits(zc[tb, tp]), _bits(zc[tb, tp + td])), (call.what, "duplicate rows differ")
        top = zc[tb, tp] == m[tb]  # (pairs, Co): the columns whose maximum the pair holds -- twice
        won = top & (call.argsel[tb] == tp[:, None])
        assert bool((won.sum(1) >= 1).all()), (call.what, "a pair of duplicate rows decides no column", c.ties[int((won.sum(1) < 1).nonzero()[0])])
        # (integer data: a row below the pair may hold the same maximum -- then it is the pick, as the first-argmax check above saw)
        low = won | ~top | (call.argsel[tb] < tp[:, None])
        assert bool(low.all()), (call.what, "tie: not the lower row (cloud, row, distance)", c.ties[int((~low).any(1).nonzero()[0])])


def check_variant(call, full, what):
    """z == NULL (with or without argsel): the bits of the storing call"""
    for name, t in T.pool_bits(call).items():
        assert torch.equal(_bits(t), _bits(getattr(full, name))), (call.what, what, name)


def check_keys(call, c):
    """the tile entry's key scratch [B][2][Co]: the minima plane is never published (a plain ReLU follows): zero after the call"""
    assert not bool(call.keys.view(c.B, 2, c.Co)[:, 1].any()), (call.what, "minima plane")


@pytest.mark.parametrize("recipe", RECIPES)
@pytest.mark.parametrize("shape", list(T.TILE_TABLE), ids=lambda s: "B%d-n%d-Ci%d-Co%d" % s)
def test_linear_forward_maxpool(shape, recipe):
    """sn_linear_forward_maxpool over its table x bias present / NULL x (z, argsel + zsel) present / NULL x the key scratch dirty with
    keys_cleared = 0 / zeroed with keys_cleared = 1."""
    c = T.pooled_case(recipe, *shape).to(DEV)
    exact, worst = recipe == "integer", {}
    for bias in (True, False):
        ref = T.pooled_ref(c, with_bias=bias)
        full = T.launch_tile(c, bias=bias).check()
        check_storing(full, c, ref, exact, worst)
        check_keys(full, c)
        same_bits(T.pool_bits(full), T.pool_bits(T.launch_tile(c, bias=bias).check()), (full.what, "second run"))
        for z, arg in ((True, True), (True, False), (False, True), (False, False)):
            for keys in ("dirty", "zeroed"):
                if (z, arg, keys) == (True, True, "dirty"):
                    continue
                v = T.launch_tile(c, z=z, arg=arg, bias=bias, keys=keys).check()
                check_variant(v, full, "against the storing call")
                check_keys(v, c)
    report("sn_linear_forward_maxpool", "%s %s (%s)" % (shape, recipe, T.TILE_TABLE[shape]), worst)


def test_maxpool_keys_cleared_by_the_narrow_rider():
    """The key scratch starts as sentinel garbage, sn_pointnet_narrow_forward's rider clears it (zero_n = B 2 Co), and
    sn_linear_forward_maxpool(keys_cleared = 1) on the narrow front's own z4 gives the bits of a keys_cleared = 0 call."""
    n = T.narrow_forward_case("real", 128).to(DEV)
    c = T.pooled_case("real", 2, 64, 128, 1024).to(DEV)
    probe = T.NetLaunch("rider keys")
    keys = probe.words64(c.B * 2 * c.Co)
    front = T.launch_narrow_forward(n, store=False, zero=keys, zero_n=c.B * 2 * c.Co).check()
    c.ain = front.z[3][:128].contiguous()
    c.coef = torch.cat([torch.ones(128, device=DEV), torch.zeros(128, device=DEV)])  # (the identity table: fmaf(z, 1, 0) = z exactly)
    c.ties = []
    via = T.launch_tile(c, keys=keys).check()
    own = T.launch_tile(c, keys="dirty").check()
    same_bits(T.pool_bits(via), T.pool_bits(own), "rider-cleared keys against keys_cleared = 0")
    check_storing(own, c, T.pooled_ref(c), False, {})


@pytest.mark.parametrize("recipe", RECIPES)
@pytest.mark.parametrize("shape", list(T.WIDE_TABLE), ids=lambda s: "R%d-n%d-Ci%d-Co%d" % s)
def test_linear_forward_maxpool_wide(shape, recipe):
    """sn_linear_forward_maxpool_wide over its table x the three template variants (z; argsel only; neither) x bias present / NULL,
    with non-identity tables (negative scales among them) and, on one row per Ci, coef_prev == NULL: the operand used as is, no ReLU.
    planes_ready = 1 with W overwritten reproduces the first call (the planes are what the kernel reads); planes_ready = 0 on the new
    W follows the new W.  One row per Ci: sn_linear_forward_maxpool on the same inputs gives the same bits."""
    from samplenet_amd._lib import lib

    R, npts, Ci, Co = shape
    sentence, also_null = T.WIDE_TABLE[shape][0], T.WIDE_TABLE[shape][5]
    assert lib.sn_linear_forward_maxpool_wide_supported(R, Ci, Co, npts) == 1
    c = T.pooled_case(recipe, R // npts, npts, Ci, Co).to(DEV)
    exact, worst = recipe == "integer", {}
    for coef in (True, False) if also_null else (True,):
        for bias in (True, False):
            ref = T.pooled_ref(c, with_bias=bias, with_coef=coef)
            full = T.launch_wide(c, bias=bias, coef=coef).check()
            check_storing(full, c, ref, exact, worst)
            same_bits(T.pool_bits(full), T.pool_bits(T.launch_wide(c, bias=bias, coef=coef).check()), (full.what, "second run"))
            for z, arg in ((False, True), (False, False)):
                check_variant(T.launch_wide(c, z=z, arg=arg, bias=bias, coef=coef).check(), full, "against the storing call")
            if coef and bias:
                first = full
            del full, ref
    # stale planes: W overwritten, planes_ready = 1 on the first call's planes
    W2 = T.other_weights(c).to(DEV)
    stale = T.launch_wide(c, W=W2, planes=first.planes_gb, planes_ready=1).check()
    same_bits(T.pool_bits(stale), T.pool_bits(first), "planes_ready = 1 must read the planes, not W")
    c2 = T.Case(**{**c.__dict__, "W": W2, "ties": []})
    fresh = T.launch_wide(c2, planes=first.planes_gb, planes_ready=0).check()
    check_storing(fresh, c2, T.pooled_ref(c2), exact, worst)
    if shape in T.WIDE_AGAINST_TILE:
        check_variant(T.launch_tile(c).check(), first, "the tile entry against the wide entry")
    report("sn_linear_forward_maxpool_wide", "%s %s (%s)" % (shape, recipe, sentence), worst)


# ---- the narrow front -----------------------------------------------------------------------------------------------------------------
def check_narrow_forward(call, c, bias, exact, worst):
    """teacher-forced: z1 against fp64 of x, W1, b1; z[l] against the fp64 layer of relu of the GPU's own z[l-1]; rows at and beyond R
    untouched in all four outputs"""
    R, b = c.R, (c.b if bias else [None] * 4)
    for t in call.z:
        assert call.filled(t[:R]) and call.untouched(t[R:]), (call.what, "rows written", tuple(t.shape))
    z, bnd = T.narrow_layer1_ref(c.x, c.W[0], b[0])
    note(worst, "z1", held(call.z[0][:R], z, bnd, exact, (call.what, "z1")))
    for l in (1, 2, 3):
        z, bnd = T.linear_ref(call.z[l - 1][:R].double().clamp_min(0), c.W[l], b[l])
        note(worst, "z%d" % (l + 1), held(call.z[l][:R], z, bnd, exact, (call.what, "z%d" % (l + 1))))


@pytest.mark.parametrize("recipe", RECIPES)
@pytest.mark.parametrize("R", list(T.NARROW_FWD_TABLE), ids=lambda r: "R%d" % r)
def test_pointnet_narrow_forward(R, recipe):
    """sn_pointnet_narrow_forward at the supported and the ragged row counts (the entry runs any R >= 1: the kernel guards ragged rows)
    x b1..b4 present / all NULL x z1..z3 stored / NULL (z4 the same bits).  planes_ready = 1 with W2..W4 AND W1 overwritten: the three
    products read the planes (z2..z4 follow the old weights given the new z1), W1 is read directly (z1 follows the new W1)."""
    from samplenet_amd._lib import lib

    assert lib.sn_pointnet_narrow_forward_supported(R, 64, 64, 64, 128) == int(T.NARROW_FWD_TABLE[R].startswith("supported"))
    c = T.narrow_forward_case(recipe, R).to(DEV)
    exact, worst = recipe == "integer", {}
    for bias in (True, False):
        full = T.launch_narrow_forward(c, bias=bias).check()
        check_narrow_forward(full, c, bias, exact, worst)
        again = T.launch_narrow_forward(c, bias=bias).check()
        bare = T.launch_narrow_forward(c, store=False, bias=bias).check()
        for l in range(4):
            assert torch.equal(_bits(full.z[l]), _bits(again.z[l])), (full.what, "not repeatable", l)
        assert torch.equal(_bits(bare.z[3]), _bits(full.z[3])), (bare.what, "z4 without z1..z3")
        if bias:
            first = full
    other = T.narrow_forward_case(recipe, R, seed=5).to(DEV)
    stale = T.launch_narrow_forward(c, W=other.W, planes=first.planes_gb, planes_ready=1).check()
    mixed = T.Case(recipe=recipe, R=R, x=c.x, W=[other.W[0]] + c.W[1:], b=c.b)
    check_narrow_forward(stale, mixed, True, exact, worst)
    fresh = T.launch_narrow_forward(c, W=other.W, planes=first.planes_gb, planes_ready=0).check()
    check_narrow_forward(fresh, T.Case(recipe=recipe, R=R, x=c.x, W=other.W, b=c.b), True, exact, worst)
    report("sn_pointnet_narrow_forward", "R %d %s (%s)" % (R, recipe, T.NARROW_FWD_TABLE[R]), worst)


@pytest.mark.parametrize("zero_n", T.NARROW_RIDER_N)
def test_pointnet_narrow_forward_rider(zero_n):
    """the zero_keys rider at R = 64 (one workgroup: 1000 words take four grid strides): words below zero_n are zero, the rest stay
    sentinel; zero_keys == NULL with zero_n = 1000 writes nothing; z4 the same bits either way"""
    c = T.narrow_forward_case("real", 64).to(DEV)
    plain = T.launch_narrow_forward(c, store=False, zero=None, zero_n=1000).check()
    probe = T.NetLaunch("rider")
    gb, view = probe.words64(1000)
    call = T.launch_narrow_forward(c, store=False, zero=(gb, view), zero_n=zero_n).check()
    assert not bool(view[:zero_n].any()), ("words below zero_n", zero_n)
    assert call.untouched(gb.view[2 * zero_n:]), ("words at and beyond zero_n", zero_n)
    assert torch.equal(_bits(call.z[3]), _bits(plain.z[3]))


@pytest.mark.parametrize("recipe", RECIPES)
@pytest.mark.parametrize("R", T.NARROW_BWD_ROWS, ids=lambda r: "R%d" % r)
def test_pointnet_narrow_backward(R, recipe):
    """sn_pointnet_narrow_backward: dx against fp64 under the bound propagated through the three products and the fma chain; z1..z3
    only as masks (signs drawn freely, planted +0.0 and -0.0 mask); planes_ready = 1 with W2..W4 overwritten reproduces the bits."""
    c = T.narrow_backward_case(recipe, R).to(DEV)
    exact, worst = recipe == "integer", {}
    dx, bnd = T.narrow_backward_ref(c)
    call = T.launch_narrow_backward(c).check()
    assert call.filled(call.dx[:R]) and call.untouched(call.dx[R:]), call.what
    note(worst, "dx", held(call.dx[:R], dx, bnd, exact, (call.what, "dx")))
    assert torch.equal(_bits(T.launch_narrow_backward(c).check().dx), _bits(call.dx)), (call.what, "not repeatable")
    other = T.narrow_backward_case(recipe, R + 1000)
    W2 = [c.W[0]] + [w.to(DEV) for w in other.W[1:]]
    stale = T.launch_narrow_backward(c, W=W2, planes=call.planes_gb, planes_ready=1).check()
    assert torch.equal(_bits(stale.dx), _bits(call.dx)), (stale.what, "planes_ready = 1 must read the planes")
    c2 = T.Case(**{**c.__dict__, "W": W2})
    fresh = T.launch_narrow_backward(c2, planes=call.planes_gb, planes_ready=0).check()
    dx2, bnd2 = T.narrow_backward_ref(c2)
    note(worst, "dx", held(fresh.dx[:R], dx2, bnd2, exact, (fresh.what, "dx after a new split")))
    report("sn_pointnet_narrow_backward", "R %d %s" % (R, recipe), worst)


# ---- the sparse data gradient through the max -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("recipe", RECIPES)
@pytest.mark.parametrize("shape", list(T.SPARSE_TABLE), ids=lambda s: "B%d-n%d-Ci%d-Co%d" % s)
def test_pool_dgrad_sparse(shape, recipe):
    """sn_pool_dgrad_sparse over its table x pick recipes (all channels of a cloud on one row; uniform; picks outside [0, npts), which
    contribute nothing) x mask operands (zprev + non-identity coef_prev; zprev alone; neither), pooled positive / negative / exactly 0:
    every element of dyprev written and held to fp64 (the early-exit chunks' zeros included)."""
    exact, worst = recipe == "integer", {}
    for pick in T.SPARSE_TABLE[shape][1]:
        c = T.sparse_case(recipe, shape, pick).to(DEV)
        for mask in T.MASKS:
            ref, bnd = T.sparse_ref(c, mask)
            call = T.launch_sparse(c, mask).check()
            assert call.filled(call.dyprev), (call.what, "elements left unwritten")
            note(worst, pick + " / " + mask, held(call.dyprev, ref, bnd, exact, call.what))
            assert torch.equal(_bits(T.launch_sparse(c, mask).check().dyprev), _bits(call.dyprev)), (call.what, "not repeatable")
            if mask != "none":  # the planted exact zeros of the mask argument, on a row that carries a gradient
                planted = call.dyprev[c.row0, :min(3, shape[2])] if mask == "zprev+coef" else call.dyprev[c.row0, 1:min(3, shape[2])]
                assert not bool(planted.any()), (call.what, "an exact zero of the mask argument let a gradient through")
        if pick == "early":
            b, ch, row = T.EARLY_HIT
            live = call.dyprev.view(shape[0], shape[1], shape[2])
            assert bool(live[b, row].any()) and not bool(live[b, 64:row].any()) and not bool(live[b + 1, 64:].any())
    report("sn_pool_dgrad_sparse", "%s %s (%s)" % (shape, recipe, T.SPARSE_TABLE[shape][0]), worst)
