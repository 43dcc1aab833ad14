"""The references, generators and tables of tests/task_net_ref.py, on the CPU (no GPU): every reference against torch's own fp64
Linear / relu / amax composition and autograd to 1e-12 relative; the three `_supported` answers, wide_group_rows, the column split and
`_scratch_bytes` restated and held to the library's host functions and to the tables' sentences; the constants against the sources;
and the conditions under which tests/test_gpu_task_net_direct.py may compare EVERY element: the integer recipes' partial sums below
2^24, the pooled layer's operand no fp32 midpoint, every ReLU argument of the sparse data gradient further from 0 than its rounding
(planted exact zeros apart), and every planted pair of duplicate rows the clear maximum of at least two columns."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import task_net_ref as T  # noqa: E402

TOL = 1e-12
RECIPES = ("integer", "real")


def close(a, b, what):
    a, b = a.detach().double(), b.detach().double()
    scale = max(float(a.abs().max()), float(b.abs().max()), 1e-300)
    assert float((a - b).abs().max()) <= TOL * scale, (what, float((a - b).abs().max()), scale)


# ---- the references -----------------------------------------------------------------------------------------------------------------
def test_pooled_reference_against_torch():
    """integer data (the operand is exact): relu(z scale + shift) -> Linear -> amax over the points -> relu; first_argmax is the lowest
    row among ties (checked against a plain loop)"""
    c = T.pooled_case("integer", 3, 192, 192, 64)
    for bias, coef in ((True, True), (False, True), (True, False)):
        z, bnd, pooled, pbnd = T.pooled_ref(c, with_bias=bias, with_coef=coef)
        a = c.ain.double()
        if coef:
            a = torch.relu(a * c.coef[:c.Ci].double() + c.coef[c.Ci:].double())
        want = torch.nn.functional.linear(a, c.W.double(), c.bias.double() if bias else None)
        close(z, want, "z")
        close(pooled, torch.relu(want.view(c.B, c.npts, c.Co).amax(1)), "pooled")
        assert bool((bnd > 0).any()) and bool((pbnd.view(c.B, 1, c.Co) >= bnd.view(c.B, c.npts, c.Co)).all())
    m, first = T.first_argmax(z.float(), c.B, c.npts)
    zc = z.float().view(c.B, c.npts, c.Co)
    ties = 0
    for b in range(c.B):
        for col in range(0, c.Co, 7):
            rows = (zc[b, :, col] == zc[b, :, col].max()).nonzero().flatten()
            ties += len(rows) > 1
            assert int(first[b, col]) == int(rows[0]) and float(m[b, col]) == float(zc[b, rows[0], col])
    assert ties > 0


def test_narrow_forward_reference_against_torch():
    c = T.narrow_forward_case("real", 33)
    for bias in (True, False):
        h, got = c.x.double(), T.narrow_forward_ref(c, with_bias=bias)
        for l in range(4):
            z = torch.nn.functional.linear(h, c.W[l].double(), c.b[l].double() if bias else None)
            close(got[l], z, "z%d" % (l + 1))
            h = torch.relu(z)
    z, bnd = T.narrow_layer1_ref(c.x, c.W[0], c.b[0])
    assert bool((bnd >= 4 * T.U * z.abs()).all())


@pytest.mark.parametrize("recipe", RECIPES)
def test_narrow_backward_reference_against_autograd(recipe):
    """dx of sum(dz4 . y4) through y = (((x W1^T . m1) W2^T . m2) W3^T . m3) W4^T with the masks m = [z > 0] held fixed; planted +0.0 and
    -0.0 both mask"""
    c = T.narrow_backward_case(recipe, 33)
    x = torch.zeros(33, 3, dtype=torch.float64, requires_grad=True)
    h = x
    for l in range(3):
        h = torch.nn.functional.linear(h, c.W[l].double()) * (c.z[l] > 0).double()
    y = torch.nn.functional.linear(h, c.W[3].double())
    (dx,) = torch.autograd.grad((y * c.dz4.double()).sum(), x)
    got, bnd = T.narrow_backward_ref(c)
    close(got, dx, "dx")
    assert bool((bnd >= 0).all()) and bool(torch.isfinite(bnd).all()) and float(bnd.max()) < 1e-2 * max(1.0, float(got.abs().max()))
    for t in c.z:
        zeros = t == 0
        assert int((zeros & ~torch.signbit(t)).sum()) >= 5 and int((zeros & torch.signbit(t)).sum()) >= 5


@pytest.mark.parametrize("pick", T.PICKS)
@pytest.mark.parametrize("mask", T.MASKS)
def test_sparse_reference_against_autograd(pick, mask):
    """y = (u . m) W^T, out[b][c] = y[b][argsel[b][c]][c] for the picks inside the cloud, loss = sum(out . [pooled > 0] g): d loss / d u"""
    shape = (2, 63, 33, 17)
    c = T.sparse_case("real", shape, pick)
    B, npts, Ci, Co = shape
    u = torch.zeros(B * npts, Ci, dtype=torch.float64, requires_grad=True)
    m = T.sparse_mask(c, mask)
    y = torch.nn.functional.linear(u if m is None else u * m, c.W.double()).view(B, npts, Co)
    arg = c.argsel.long()
    inside = (arg >= 0) & (arg < npts)
    out = torch.gather(y, 1, arg.clamp(0, npts - 1)[:, None, :])[:, 0]
    gsel = torch.where((c.pooled > 0) & inside, c.g, torch.zeros_like(c.g)).double()
    (du,) = torch.autograd.grad((out * gsel).sum(), u)
    got, bnd = T.sparse_ref(c, mask)
    close(got, du, "dyprev")
    assert bool((bnd >= 0).all())
    if pick == "outside":
        assert int((~inside).sum()) >= 10
    assert bool((c.pooled > 0).any()) and bool((c.pooled < 0).any()) and bool((c.pooled == 0).any())


# ---- the host functions, the constants, the tables -----------------------------------------------------------------------------------
def test_constants_in_the_sources():
    k = T.source_constants()
    assert (k["kWideRows"], k["kWideBN"], k["kNarrowRows"]) == (128, 64, 128)
    assert (k["kPdsThreads"], k["kPdsGroups"], k["kPdsCi"], k["kPdsPts"], k["kPdsCh"]) == (512, 16, 32, 64, 32)
    assert (k["TileBig::BM"], k["TileBig::BN"], k["BK"]) == (64, 64, 64)


def test_route_predicates_in_the_sources():
    """The predicates and index expressions the restatements and the tables were read from still stand in the sources as read."""
    found = T.source_routes()
    assert all(n == 1 for n in found.values()), {k: n for k, n in found.items() if n != 1}


def test_supported_answers_and_scratch_bytes():
    from samplenet_amd._lib import lib

    for R in (0, 64, 128, 192, 16256, 16384, 16448, 16512, 32768):
        for npts in (0, 16, 32, 48, 64, 96, 128, 192, 1024):
            for Ci in (32, 64, 96, 128, 192, 256):
                for Co in (64, 448, 512, 544, 576, 1024):
                    assert lib.sn_linear_forward_maxpool_supported(R, Ci, Co, npts) == int(npts > 0 and T.tile_supported(R, Ci, Co, npts)), (R, Ci, Co, npts)
                    ok = npts > 0 and T.wide_supported(R, Ci, Co, npts)
                    assert lib.sn_linear_forward_maxpool_wide_supported(R, Ci, Co, npts) == int(ok), (R, Ci, Co, npts)
                    if ok:
                        assert lib.sn_linear_forward_maxpool_wide_scratch_bytes(R, Ci, Co, npts) == T.wide_scratch_bytes(R, Co, npts)
    for B, npts, Ci, Co in ((1, 1, 1, 1), (32, 256, 128, 1024), (1, 257, 8, 8), (0, 8, 8, 8), (1, 0, 8, 8), (1, 8, 0, 8), (1, 8, 8, 0), (-1, 8, 8, 8)):
        assert lib.sn_pool_dgrad_sparse_supported(B, npts, Ci, Co) == int(T.sparse_supported(B, npts, Ci, Co)), (B, npts, Ci, Co)
    for R in (0, 1, 63, 64, 65, 128, 150, 4160):
        assert lib.sn_pointnet_narrow_forward_supported(R, 64, 64, 64, 128) == int(R >= 64 and R % 64 == 0)
        assert lib.sn_pointnet_narrow_backward_supported(R, 64, 64, 64, 128) == int(R >= 1)
    assert lib.sn_pointnet_narrow_forward_supported(128, 64, 64, 64, 64) == 0 and lib.sn_pointnet_narrow_backward_supported(128, 64, 128, 64, 128) == 0


def test_tables_against_their_sentences():
    from samplenet_amd._lib import lib

    for (B, npts, Ci, Co), sentence in T.TILE_TABLE.items():
        assert T.tile_supported(B * npts, Ci, Co, npts), (B, npts, Ci, Co)
        tiles = npts // 64
        assert {1: "one tile", 2: "two tiles", 3: "three tiles"}[tiles] in sentence or Co == 1024, sentence
    assert {s[2] for s in T.TILE_TABLE} == {64, 128, 192} and {s[3] for s in T.TILE_TABLE} == {64, 128, 1024}
    for (R, npts, Ci, Co), (sentence, group, partials, cs, nblk, _) in T.WIDE_TABLE.items():
        assert T.wide_supported(R, Ci, Co, npts) and lib.sn_linear_forward_maxpool_wide_supported(R, Ci, Co, npts) == 1
        assert group == T.wide_group_rows(npts) == min(group, npts) and partials == npts // group and cs == T.wide_column_split(R, Co)
        assert nblk == Co // cs // 64
        assert lib.sn_linear_forward_maxpool_wide_scratch_bytes(R, Ci, Co, npts) == (R // npts) * partials * Co * 8
        straddle = 128 % npts != 0 and npts % 128 != 0  # a workgroup's 128 rows hold a cloud's end that is not theirs
        assert ("straddl" in sentence) == straddle, sentence
        if "group" in sentence:
            assert "group %d" % group in sentence, sentence
        assert ("no split" in sentence) == (cs == 1) and ("split in two" not in sentence or cs == 2), sentence
        if "partial" in sentence:
            assert {1: "one partial", 3: "three partials", 8: "eight partials"}[partials] in sentence, sentence
        if "row blocks" in sentence:
            assert "%d row blocks" % (R // 128) in sentence
        if "column blocks" in sentence:
            assert nblk == 9 and nblk % 2 == 1 and R // 128 // 8 > nblk  # (rot = (block / 8) % nblk passes nblk: it wraps)
    assert {s[2] for s in T.WIDE_AGAINST_TILE} == {64, 128} and all(T.tile_supported(s[0], s[2], s[3], s[1]) for s in T.WIDE_AGAINST_TILE)
    assert {s[2] for s, v in T.WIDE_TABLE.items() if v[5]} == {64, 128}  # coef_prev == NULL on one row per Ci
    for R, sentence in T.NARROW_FWD_TABLE.items():
        assert sentence.startswith("supported") == (R >= 64 and R % 64 == 0), R
    assert T.NARROW_RIDER_N[-1] > 3 * 256  # one workgroup of 256 threads: four strides
    for (B, npts, Ci, Co), (sentence, picks) in T.SPARSE_TABLE.items():
        assert T.sparse_supported(B, npts, Ci, Co)
        chunks, passes = (npts + 63) // 64, (Co + 16 * 32 - 1) // (16 * 32)
        if "chunks" in sentence and "four" in sentence:
            assert chunks == 4 and passes == 2 and Co % 512 == 1
        if "second row chunk of one row" in sentence:
            assert chunks == 2 and npts % 64 == 1 and passes == 1 and Co == 512
        if "ragged" in sentence:
            assert npts % 64 and Ci % 32 == 1 and Co == 17
        if "one channel per group" in sentence:
            assert Co == 16
        if "early" in picks:
            assert chunks == 4 and T.EARLY_HIT[2] == npts - 1 and T.EARLY_HIT[0] < B and T.EARLY_HIT[1] < Co


# ---- the generators' conditions --------------------------------------------------------------------------------------------------------
def _pooled_combos(table_row_null):
    return [(b, k) for k in ((True, False) if table_row_null else (True,)) for b in (True, False)]


def _ties_win(c, z, slack):
    """every planted pair holds the maximum of >= 2 columns, the best other row further below than `slack`"""
    zc = z.view(c.B, c.npts, c.Co)
    top = zc.topk(3, dim=1).values  # (B, 3, Co)
    tb, tp, td = (torch.tensor(col) for col in zip(*c.ties))
    zp = zc[tb, tp]
    assert float((zp - zc[tb, tp + td]).abs().max()) <= 1e-9 * float(zp.abs().max())
    wins = (zp >= top[tb, 0] - slack / 4) & (top[tb, 2] < zp - slack)
    assert int(wins.sum(1).min()) >= 2, (c.recipe, c.B, c.npts, c.Ci, c.Co, int(wins.sum(1).min()))


@pytest.mark.parametrize("recipe", RECIPES)
@pytest.mark.parametrize("entry", ("tile", "wide"))
def test_pooled_generator_conditions(entry, recipe):
    table = T.TILE_TABLE if entry == "tile" else T.WIDE_TABLE
    dist = set()
    for shape, val in table.items():
        B, npts, Ci, Co = shape if entry == "tile" else (shape[0] // shape[1], shape[1], shape[2], shape[3])
        c = T.pooled_case(recipe, B, npts, Ci, Co)
        assert c.ties[0][:2] == (0, 0) and len({(b, r) for b, p, d in c.ties for r in (p, p + d)}) == 2 * len(c.ties)
        assert all(0 <= p and p + d < npts for b, p, d in c.ties)
        dist |= {d for b, p, d in c.ties}
        for with_coef in ((True, False) if entry == "wide" and val[5] else (True,)):
            a = T.operand(c.ain, c.coef if with_coef else None)
            if recipe == "integer":  # every partial sum an integer below 2^24; neither operand has a third bf16 plane, so the six
                # products of a k-step hold all four that are not zero
                from skinny_ref import split3_ref

                assert bool((a == a.round()).all()) and set(c.W.unique().tolist()) <= {-1.0, 0.0, 1.0, 257.0}
                assert not bool(split3_ref(a.float())[2].any()) and not bool(split3_ref(c.W)[2].any())
                assert bool(split3_ref(a.float())[1].any()) and bool(split3_ref(c.W)[1].any())
                assert int((a.abs() @ c.W.double().abs().t()).max().long()) + int(c.bias.abs().max().long()) < 2 ** 24
            elif with_coef:
                assert T.operand_midpoints(c.ain, c.coef) == 0
                assert bool((c.coef[:Ci] < 0).any()) and bool((c.coef[:Ci] > 0).any())
            for with_bias in (True, False):
                z = a @ c.W.double().t() + (c.bias.double() if with_bias else 0.0)
                slack = 2 * (Ci + 8) * T.U * (float(a.abs().sum(1).max()) * float(c.W.abs().max()) + float(c.bias.abs().max()))
                _ties_win(c, z, 0.5 if recipe == "integer" else slack)  # (integers are compared exactly: any gap is clear)
    assert dist == set(T.TIE_DISTANCES)


@pytest.mark.parametrize("R", sorted(set(T.NARROW_FWD_TABLE) | set(T.NARROW_BWD_ROWS)))
def test_narrow_integer_ranges(R):
    """integer recipes: the magnitude sums |x| |W1| |W2| ... (every partial sum's bound) stay below 2^24, forward and backward"""
    if R in T.NARROW_FWD_TABLE:
        c = T.narrow_forward_case("integer", R)
        m = c.x.double().abs()
        for l in range(4):
            assert set(c.W[l].unique().tolist()) <= {-1.0, 0.0, 1.0}
            m = m @ c.W[l].double().abs().t() + c.b[l].double().abs()
            assert int(m.max().long()) < 2 ** 24, (R, l)
    if R in T.NARROW_BWD_ROWS:
        c = T.narrow_backward_case("integer", R)
        m = c.dz4.double().abs()
        for l in (3, 2, 1, 0):
            m = m @ c.W[l].double().abs()
            assert int(m.max().long()) < 2 ** 24, (R, l)


@pytest.mark.parametrize("shape", list(T.SPARSE_TABLE), ids=lambda s: "B%d-n%d-Ci%d-Co%d" % s)
def test_sparse_generator_conditions(shape):
    B, npts, Ci, Co = shape
    for pick in T.SPARSE_TABLE[shape][1]:
        c = T.sparse_case("integer", shape, pick)
        assert 3 * Co < 2 ** 24 and float(c.g.abs().max()) <= 3 and set(c.W.unique().tolist()) <= {-1.0, 0.0, 1.0}
        c = T.sparse_case("real", shape, pick)
        for mask in ("zprev+coef", "zprev"):
            t, mag = T.sparse_mask_argument(c, mask)
            zero = t == 0
            assert bool((t.abs() > 4 * T.U * mag)[~zero].all()), (shape, pick, mask)
            planted = [(c.row0, j) for j in range(min(3, Ci))] if mask == "zprev+coef" else [(c.row0, j) for j in range(1, min(3, Ci))]
            assert sorted(map(tuple, zero.nonzero().tolist())) == sorted(planted), (shape, pick, mask)
        inside = (c.argsel >= 0) & (c.argsel < npts)
        if pick == "outside":
            assert bool((~inside).any()) and bool((c.argsel < 0).any()) and (B * Co < 2 or bool((c.argsel >= npts).any()))
        if pick == "early":
            b, ch, row = T.EARLY_HIT
            far = c.argsel >= 64
            assert int(far.sum()) == 1 and int(c.argsel[b, ch]) == row and float(c.pooled[b, ch]) > 0 and float(c.g[b, ch]) != 0
        if pick == "one row":
            assert bool((c.argsel == c.argsel[:, :1]).all())
