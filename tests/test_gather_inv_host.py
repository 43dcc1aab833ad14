"""tests/gather_inv_ref.py, the yardstick of sn_gather_invert and sn_weighted_gather_backward_inverted, held to numpy's stable
argsort, to its own float64 twin's counted bound and to float64 torch autograd; the proof that a list walked in the wrong order
shows in the bits (so the GPU test can see an order error); the recipes' promises; the shape table against the kernels' constants;
and the host half of the two entries' contract: the prototypes, the exports, the support predicate, argument errors and no-op
cases in a child process that sees no GPU, ValueError / RuntimeError from the Python surface.  No GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

import gather_inv_ref as G
from cabi_runner import check_case, run_cases


@pytest.mark.parametrize("recipe", G.INDEX_RECIPES)
def test_invert_is_the_stable_argsort(recipe):
    for shape in G.SHAPES:
        b, c, n, m, k = shape
        ref = G.case(shape, recipe)
        idx = ref["idx"].reshape(b, -1).astype(np.int64)
        for i in range(b):
            valid = (idx[i] >= 0) & (idx[i] < n)
            key = np.where(valid, idx[i], n)                        # the invalid entries sort behind every row
            want = np.argsort(key, kind="stable")[:valid.sum()]
            nv = int(valid.sum())
            assert ref["start"][i, n] == nv and np.array_equal(ref["order"][i, :nv], want) and (ref["order"][i, nv:] == -1).all()
            assert np.array_equal(ref["start"][i], np.concatenate([[0], np.cumsum(np.bincount(idx[i][valid], minlength=n))]))
        assert ref["start"].dtype == np.int32 and ref["order"].dtype == np.int32


@pytest.mark.parametrize("values", G.VALUE_RECIPES)
@pytest.mark.parametrize("recipe", G.INDEX_RECIPES)
def test_float32_sum_stays_within_the_counted_bound(recipe, values):
    worst = 0.0
    for shape in G.SHAPES:
        ref = G.case(shape, recipe, values)
        err = np.abs(ref["grad32"].astype(np.float64) - ref["grad64"])
        assert (err <= ref["bound"]).all(), shape
        if values == "int":
            assert np.array_equal(ref["grad32"].astype(np.float64), ref["grad64"]), shape   # exact: the bound is not needed
        pos = ref["bound"] > 0
        if pos.any():
            worst = max(worst, float((err[pos] / ref["bound"][pos]).max()))
    print("%s / %s: worst error / bound %.3g" % (recipe, values, worst))


def test_float64_twin_is_the_gradient_of_the_gather():
    shape = (2, 16, 65, 257, 3)
    b, c, n, m, k = shape
    for recipe in ("nn", "oob"):
        ref = G.case(shape, recipe, "mixed")
        idx = torch.tensor(ref["idx"].astype(np.int64)).view(b, 1, m * k)
        valid = (idx >= 0) & (idx < n)
        X = torch.zeros(b, c, n, dtype=torch.float64, requires_grad=True)
        f = torch.gather(X, 2, idx.clamp(0, n - 1).expand(b, c, m * k)) * valid            # an invalid entry gathers nothing
        out = (f.view(b, c, m, k) * torch.tensor(ref["weights"]).double()[:, None]).sum(-1)
        (gX,) = torch.autograd.grad(out, [X], torch.tensor(ref["grad_out"]).double())
        scale = np.abs(ref["grad64"]).max()
        assert np.allclose(gX.numpy(), ref["grad64"], rtol=0, atol=1e-12 * scale)


def test_a_reversed_walk_shows_in_the_bits():
    """On the mixed-magnitude values, summing each list backwards gives other bits than summing it forwards on at least one element
    of every shape row that has a list longer than 2 (two terms commute)."""
    for shape in G.SHAPES:
        b, c, n, m, k = shape
        longest, differs = 0, 0
        for recipe in G.INDEX_RECIPES:
            ref = G.case(shape, recipe, "mixed")
            longest = max(longest, int(np.diff(ref["start"].astype(np.int64), axis=1).max()))
            back = G.backward32(c, n, k, ref["weights"], ref["grad_out"], ref["start"], ref["order"], reverse=True)
            differs += int((back.view(np.int32) != ref["grad32"].view(np.int32)).sum())
            assert (np.abs(back.astype(np.float64) - ref["grad64"]) <= ref["bound"]).all()  # (another order, the same bound)
        assert longest > 2, shape   # every row of the table has such a list
        assert differs > 0, shape


def test_the_recipes_reach_what_they_promise():
    for shape in G.SHAPES:
        b, c, n, m, k = shape
        count = {r: np.diff(G.case(shape, r)["start"].astype(np.int64), axis=1) for r in G.INDEX_RECIPES}
        idx = {r: G.case(shape, r)["idx"] for r in G.INDEX_RECIPES}
        for r in ("nn", "same", "uniform", "descending", "empty"):
            assert ((idx[r] >= 0) & (idx[r] < n)).all() and (count[r].sum(1) == m * k).all(), (shape, r)
        assert (idx["same"] == ((np.arange(k) % 3) % n)).all() and (count["same"][:, 3:] == 0).all()
        flat = idx["descending"].reshape(b, -1)
        assert (np.diff(flat, axis=1) <= 0).all() and flat[0, 0] == (m * k - 1) * n // (m * k)
        assert ((idx["oob"] == -1) | (idx["oob"] == n) | ((idx["oob"] >= 0) & (idx["oob"] < n))).all()
        if n >= 2:
            assert (count["empty"][:, 1::2] == 0).all()
    big = G.case((1, 5, 4, 4100, 3), "oob")["idx"]
    assert (big == -1).any() and (big == 4).any() and 0.05 < ((big < 0) | (big >= 4)).mean() < 0.15
    assert (np.diff(G.case((1, 5, 4, 4100, 3), "uniform")["start"].astype(np.int64), axis=1) > 2900).all()  # lists of about 3000
    assert (G.case((2, 3, 2, 5, 3), "nn")["idx"][:, :, 2] == 0).all()                                     # the m < 3 filling
    for values in G.VALUE_RECIPES:
        w, g = G.make_values((1, 17, 64, 64, 3), values)
        assert w.dtype == g.dtype == np.float32 and w.shape == (1, 64, 3) and g.shape == (1, 17, 64)
    w, g = G.make_values((1, 17, 64, 64, 3), "int")
    assert np.array_equal(w, np.round(w)) and np.abs(w).max() <= 3 and np.abs(g).max() <= 3
    w, g = G.make_values((1, 5, 4, 4100, 3), "mixed")
    assert np.abs(w).max() / np.median(np.abs(w)) > 20    # magnitudes are mixed


def test_the_table_reaches_every_branch_of_the_kernels():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "samplenet_amd", "csrc", "feature_propagate.hip")).read()
    for line, value in (("constexpr int kInvTile = 4096;", G.TILE), ("constexpr int kGbChannels = 8;", G.CHANNELS),
                        ("constexpr long long kInvWork = 1ll << 26;", G.WORK)):   # the constants as the kernels' source spells them
        assert src.count(line) == 1, line
        spelled = line.split(" = ")[1].rstrip(";")
        assert (1 << int(spelled.split("<<")[1]) if "<<" in spelled else int(spelled)) == value, line
    ns, cs, ks = {s[2] for s in G.SHAPES}, {s[1] for s in G.SHAPES}, {s[4] for s in G.SHAPES}
    assert {1, 64, 65, G.TILE + 1, 16385} <= ns and any(n > 4 * G.TILE for n in ns)
    assert any(c % G.CHANNELS for c in cs) and any(c > G.CHANNELS and c % G.CHANNELS for c in cs) and any(c < G.CHANNELS for c in cs)
    assert {1, 3, 8} <= ks and any(s[0] > 64 for s in G.SHAPES)
    assert all(G.supported(s[2], s[3] * s[4]) for s in G.SHAPES)


# ------------------------------------------------------------------------------------------------ the entries, no GPU
BAD, UNSUPPORTED = 10001, 10002
P_ = "PTR"  # a non-NULL device pointer that is never dereferenced
I_BASE = [2, 8, 12, P_, P_, P_, None]                              # sn_gather_invert
B_BASE = [2, 5, 8, 4, 3, P_, P_, P_, P_, P_, None]                 # sn_weighted_gather_backward_inverted
PAST = (1 << 20, 4097)                                             # 16384 groups of 64 rows * 4097 entries = 2^26 + 16384


def _with(base, changes):
    out = list(base)
    for k, v in changes.items():
        out[k] = v
    return out


def _cases():
    q, w = "sn_gather_invert", "sn_weighted_gather_backward_inverted"
    out = []
    for pos in (0, 1, 2):
        out.append(("%s-negative-%d" % (q, pos), q, _with(I_BASE, {pos: -1}), BAD, "negative size"))
    for pos in (3, 4, 5):
        out.append(("%s-null-%d" % (q, pos), q, _with(I_BASE, {pos: None}), BAD, "null pointer"))
    out.append((q + "-past-the-bound", q, _with(I_BASE, {1: PAST[0], 2: PAST[1]}), UNSUPPORTED, "sn_gather_invert_supported"))
    out.append((q + "-null-before-the-bound", q, _with(I_BASE, {1: PAST[0], 2: PAST[1], 4: None}), BAD, "null pointer"))
    nq = I_BASE[:3] + [None] * 4
    for tag, ch in (("b0", {0: 0}), ("n0", {1: 0})):       # the documented no-ops: nothing dereferenced, nothing launched
        out.append((q + "-noop-" + tag, q, _with(nq, ch), 0, None))
    for pos in (0, 1, 2, 3):
        out.append(("%s-negative-%d" % (w, pos), w, _with(B_BASE, {pos: -1}), BAD, "bad size"))
    out.append((w + "-k0", w, _with(B_BASE, {4: 0}), BAD, "bad size"))
    out.append((w + "-mk-overflow", w, _with(B_BASE, {3: 1 << 30, 4: 2}), BAD, "31 bits"))
    for pos in (5, 6, 7, 8, 9):
        out.append(("%s-null-%d" % (w, pos), w, _with(B_BASE, {pos: None}), BAD, "null pointer"))
    out.append((w + "-too-many-workgroups", w, _with(B_BASE, {0: 1 << 20, 1: 1 << 20, 2: 1 << 20}), UNSUPPORTED, "workgroups"))
    nw = B_BASE[:5] + [None] * 6
    for tag, ch in (("b0", {0: 0}), ("c0", {1: 0}), ("n0", {2: 0})):
        out.append((w + "-noop-" + tag, w, _with(nw, ch), 0, None))
    return out


CASES = _cases()


@pytest.fixture(scope="module")
def results():
    return run_cases(CASES)


def test_the_header_declares_and_the_library_exports_both_entries():
    from samplenet_amd import _lib

    header = open(_lib.HEADERS[1]).read()
    for name, base in (("sn_gather_invert", I_BASE), ("sn_weighted_gather_backward_inverted", B_BASE)):
        assert ("int %s(" % name) in header, name
        assert hasattr(_lib.lib, name), name
        proto = _lib.PROTOTYPES[name]
        assert len(proto) == len(base) and _lib.RESTYPES[name] is ctypes.c_int, name
        for ty, a in zip(proto, base):
            assert (ty is ctypes.c_void_p) == (a is None or a == P_), name
    assert _lib.PROTOTYPES["sn_gather_invert_supported"] == [ctypes.c_int, ctypes.c_int]
    assert len({c[0] for c in CASES}) == len(CASES)


def test_the_support_predicate_is_the_documented_bound():
    from samplenet_amd import ops
    from samplenet_amd._lib import lib

    for n, ne in [(0, 0), (1, 1), (64, 1 << 26), (64, (1 << 26) + 1), (65, 1 << 25), (65, (1 << 25) + 1), (16385, 3 * 4096),
                  (16385, 261123), (16385, 261124), PAST, (PAST[0], PAST[1] - 1), (2 ** 31 - 2, 0), (2 ** 31 - 1, 0)]:
        want = G.supported(n, ne) and n < 2 ** 31 - 1
        assert bool(lib.sn_gather_invert_supported(n, ne)) == want == ops.gather_invert_supported(n, ne), (n, ne)
    assert lib.sn_gather_invert_supported(16385, 3 * 4096) == 1                        # what a bound must admit
    assert lib.sn_gather_invert_supported(-1, 4) == 0 and lib.sn_gather_invert_supported(4, -1) == 0
    assert not ops.gather_invert_supported(2 ** 31, 1) and not ops.gather_invert_supported(1, 2 ** 31)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_argument_table(results, case):
    check_case(results, case)


def test_the_python_surface_refuses_what_it_cannot_serve():
    from samplenet_amd import ops

    idx = torch.zeros(1, 8, 3, dtype=torch.int32)
    with pytest.raises(RuntimeError):
        ops.gather_invert(idx, 4)                               # a CPU tensor: no CPU route exists
    with pytest.raises(RuntimeError):
        ops.three_interpolate(torch.zeros(1, 5, 4), idx, torch.zeros(1, 8, 3), inverse=None)
    assert ops.GatherInverse._fields == ("start", "order")
