"""sn_retrieval_metrics called directly, every output in guarded buffers (tests/cabi_ref.py), against the numpy restatement of
tests/retrieval_ref.py (held to the contract's worked example by tests/test_retrieval_host.py).

Grid recipes (distances exact in float32 in any order): `order`, `n_relevant` and `sorted_dist` bit for bit against the float64
reference, `ap` and `prec` equal to the reference's float64 value rounded to float32, d(i, j) == d(j, i) -- at one shape per branch:
n = 1, 2, 3 (no rank, one rank, the smallest tie), 64 / 65 and 1024 / 1025 (the padded power of two), 2468 (two queries per
workgroup), 8192 (one; the limit), C = 1, 3, 255, 256, 257 (the lanes' tail), S = 1, 3, L = 1, 20, 64.  At n = 8192 the numpy
reference covers every 16th query and the last (the whole set costs numpy ~8 s); what holds for ALL queries there is checked on the
device: every ranking is a permutation of the others, ascends strictly in (distance bits, index), and the distances are symmetric.

Real-valued recipe: `sorted_dist` equals the float32 restatement bit for bit and lies within the counted bound of float64; `ap` /
`prec` are the float64 formulas on the device's own order.  Near-ties may order differently from float64: the resulting difference
in mean average precision is printed and recorded in profiles/retrieval/errors.txt, not asserted."""
import itertools
import os

import numpy as np
import pytest
import torch

import cabi_ref as G
import retrieval_ref as R

pytestmark = pytest.mark.gpu

NAMES = ("ap", "prec", "n_relevant", "order", "sorted_dist")
ALL = (True,) * 5


def _lib():
    from samplenet_amd._lib import check, lib

    return lib, check


def call(desc, labels, L, want=ALL):
    """-> the five outputs as device tensors (None where not wanted); inputs and guards verified"""
    lib, check = _lib()
    S, n, C = desc.shape
    m = max(n - 1, 0)
    gd, gl = G.Guarded(desc.shape, fill=desc), G.Guarded((n,), torch.int32, fill=labels)
    shapes = [((S, n), torch.float32), ((S, n, L), torch.float32), ((n,), torch.int32), ((S, n, m), torch.int32), ((S, n, m), torch.float32)]
    outs = [G.Guarded(sh, dt) if w else None for (sh, dt), w in zip(shapes, want)]
    assert lib.sn_workspace_bytes(b"retrieval_metrics", S, n, C, L) == 0
    check(lib.sn_retrieval_metrics(S, n, C, gd.ptr(), gl.ptr(), L, *[G.arg(o) for o in outs], None, None), "sn_retrieval_metrics")
    torch.cuda.synchronize()
    assert gd.guards_intact() and gl.guards_intact()
    assert np.array_equal(gd.numpy().view(np.int32), desc.view(np.int32)) and np.array_equal(gl.numpy(), labels)
    return [None if o is None else o.check("sn_retrieval_metrics") for o in outs]


def on_device(od, sd):
    """for ALL queries: a permutation of the others, strictly ascending in (distance bits, index), symmetric distances"""
    S, n, m = od.shape
    if m == 0:
        return
    idx, bits = od.long(), sd.view(torch.int32)
    assert int(idx.min()) >= 0 and int(idx.max()) < n
    seen = torch.zeros(S, n, n, dtype=torch.bool, device=od.device).scatter_(2, idx, True)
    assert torch.equal(seen, ~torch.eye(n, dtype=torch.bool, device=od.device).expand(S, n, n))
    del seen
    a, b = bits[..., :-1], bits[..., 1:]
    assert int(bits.min()) >= 0  # sums of squares: +0 and above (a NaN's pattern lies above every number's)
    assert bool(((a < b) | ((a == b) & (od[..., :-1] < od[..., 1:]))).all())
    D = torch.full((S, n, n), -1, dtype=torch.int32, device=od.device).scatter_(2, idx, bits)
    assert torch.equal(D, D.transpose(1, 2)), "d(i, j) != d(j, i)"


def against_grid_reference(desc, labels, L, got, rows=None):
    ap, prec, nrel, od, sd = got
    S, n, _ = desc.shape
    on_device(od, sd)
    sel = np.arange(n) if rows is None else np.asarray(rows)
    dev_rows = torch.from_numpy(sel).to(od.device)
    assert nrel.dtype == torch.int32 and od.dtype == torch.int32
    for s in range(S):
        ref = R.reference(desc[s], labels, L, exact_grid=True, rows=sel)
        o, d = od[s][dev_rows].cpu().numpy(), sd[s][dev_rows].cpu().numpy()
        assert np.array_equal(o, ref["order"]), "set %d: first difference at %s" % (s, np.argwhere(o != ref["order"])[:1])
        assert R.order_is_the_ranking(ref["d"], o, sel)
        assert d.dtype == np.float32 and np.array_equal(d.astype(np.float64), ref["sorted_dist"]) and not np.signbit(d).any()
        assert np.array_equal(nrel.cpu().numpy()[sel], ref["n_relevant"])
        a, p = ap[s].cpu().numpy()[sel], prec[s].cpu().numpy()[sel]
        assert np.array_equal(a, ref["ap"].astype(np.float32), equal_nan=True), np.argwhere(a != ref["ap"].astype(np.float32))[:4]
        assert np.array_equal(p, ref["prec"].astype(np.float32), equal_nan=True)
    return ref


# (C = 257 is one square past the recipe's 256: a sum of at most 4112, 21 bits -- still exact)
@pytest.mark.parametrize("n,C,S,L,classes", [(1, 1, 1, 1, 2), (2, 3, 3, 20, 1), (3, 255, 1, 64, 2), (64, 256, 3, 20, 5), (65, 257, 1, 64, 3),
                                             (65, 1, 3, 1, 4), (1024, 256, 1, 20, 40), (1025, 3, 3, 64, 7), (2468, 256, 1, 20, 40),
                                             (8192, 4, 1, 20, 3)])
def test_grid_shapes(n, C, S, L, classes):
    desc, labels = R.make_case("grid", S, n, C, classes)
    rows = None if n <= 4096 else np.unique(np.r_[np.arange(0, n, 16), n - 1])
    got = call(desc, labels, L)
    against_grid_reference(desc, labels, L, got, rows)
    if n == 1:
        assert np.isnan(got[0].cpu().numpy()).all() and np.isnan(got[1].cpu().numpy()).all() and int(got[2][0]) == 0
    valid = got[2].cpu().numpy() > 0
    assert np.array_equal(np.isnan(got[0].cpu().numpy()), np.broadcast_to(~valid, (S, n)))   # every query, also past the reference's rows
    assert np.array_equal(np.isnan(got[1].cpu().numpy()), np.broadcast_to(~valid[None, :, None], (S, n, L)))
    assert np.array_equal(got[2].cpu().numpy(), np.bincount(labels, minlength=classes)[labels] - 1)


@pytest.mark.parametrize("recipe", R.RECIPES[1:])
@pytest.mark.parametrize("n,C,S,L", [(3, 1, 1, 1), (65, 255, 3, 20), (1025, 3, 1, 64)])
def test_grid_recipes(recipe, n, C, S, L):
    desc, labels = R.make_case(recipe, S, n, C)
    got = call(desc, labels, L)
    against_grid_reference(desc, labels, L, got)
    ap, prec, nrel, od, sd = [g.cpu().numpy() for g in got]
    if recipe == "identical":  # every distance ties: the index alone orders
        assert (sd == 0).all() and np.array_equal(od, np.broadcast_to([[j for j in range(n) if j != i] for i in range(n)], od.shape))
    if recipe == "duplicates":
        # the first and the last shape are one: a zero distance in front of both rankings, index 0 the lowest there can be
        assert (sd[:, 0, 0] == 0).all() and (sd[:, n - 1, 0] == 0).all() and (od[:, n - 1, 0] == 0).all()
        assert n <= 3 or (sd[..., 0] != 0).any()
    if recipe == "one_label":
        assert (nrel == n - 1).all() and (ap == 1).all() and (prec == 1).all()
    if recipe == "distinct_labels":
        assert (nrel == 0).all() and np.isnan(ap).all() and np.isnan(prec).all()
    if recipe == "singleton":
        assert nrel[n // 2] == 0 and np.isnan(ap[:, n // 2]).all() and np.isnan(prec[:, n // 2]).all()
        if n > 3:
            assert np.isnan(ap).sum() == S


@pytest.mark.parametrize("S,n,C,L", [(2, 65, 3, 7), (1, 1025, 5, 20)])
def test_every_null_output_combination(S, n, C, L):
    desc, labels = R.make_case("duplicates", S, n, C, classes=3)
    full = [g.cpu().numpy() for g in call(desc, labels, L)]
    for want in itertools.product((False, True), repeat=5):
        got = call(desc, labels, L, want)
        for w, a, b, name in zip(want, got, full, NAMES):
            assert (a is None) if not w else np.array_equal(a.cpu().numpy().view(np.int32), b.view(np.int32)), (want, name)
    # the labels are not read when no score is wanted
    lib, check = _lib()
    gd, od = G.Guarded(desc.shape, fill=desc), G.Guarded((S, n, n - 1), torch.int32)
    check(lib.sn_retrieval_metrics(S, n, C, gd.ptr(), None, L, None, None, None, od.ptr(), None, None, None), "order alone")
    torch.cuda.synchronize()
    assert np.array_equal(od.check().cpu().numpy(), full[3])


def test_limits_and_empty_cases():
    lib, check = _lib()
    S, n, C, L = 2, 8, 3, 4
    desc, labels = R.make_case("grid", S, n, C)
    gd, gl = G.Guarded(desc.shape, fill=desc), G.Guarded((n,), torch.int32, fill=labels)
    outs = [G.Guarded((S, n)), G.Guarded((S, n, L)), G.Guarded((n,), torch.int32), G.Guarded((S, n, n - 1), torch.int32), G.Guarded((S, n, n - 1))]
    o = [x.ptr() for x in outs]
    run = lambda S_, n_, C_, L_, d=gd.ptr(), lab=gl.ptr(), out=o: lib.sn_retrieval_metrics(S_, n_, C_, d, lab, L_, *out, None, None)  # noqa: E731
    # no-ops
    check(run(0, n, C, L), "S = 0")
    check(run(S, 0, C, L), "n = 0")
    check(run(0, 0, C, L, None, None, [None] * 5), "S = n = 0, no pointers")
    check(run(S, n, C, L, out=[None] * 5), "no output wanted")
    # refused with a message, before any device work
    for bad, code in (((S, 8193, C, L), G.UNSUPPORTED), ((S, n, C, 65), G.UNSUPPORTED), ((65536, n, C, L), G.UNSUPPORTED),
                      ((S, n, 0, L), G.BAD_ARGUMENT), ((S, n, C, 0), G.BAD_ARGUMENT), ((-1, n, C, L), G.BAD_ARGUMENT),
                      ((S, -1, C, L), G.BAD_ARGUMENT)):
        assert run(*bad) == code, bad
        assert lib.sn_last_error_string().startswith(b"sn_retrieval_metrics"), bad
    assert run(1, 8193, C, L) == G.UNSUPPORTED and b"n <= 8192" in lib.sn_last_error_string()
    assert run(S, n, C, L, d=None) == G.BAD_ARGUMENT
    assert run(S, n, C, L, lab=None) == G.BAD_ARGUMENT
    torch.cuda.synchronize()
    assert all(x.untouched() for x in outs) and gd.guards_intact() and gl.guards_intact()
    assert lib.sn_workspace_bytes(b"retrieval_metrics", 11, 8192, 256, 64) >= 0
    # n = 8192 and L = 64 themselves are taken (test_grid_shapes runs n = 8192); S, n, C, L = 2, 8, 3, 4 runs
    check(run(S, n, C, L), "plain")
    torch.cuda.synchronize()
    assert all(x.guards_intact() and x.fully_written() for x in outs)


_ERRORS = {}


def _record(classes, n, C, diff, map_dev, map_64, swapped):
    _ERRORS[classes] = ("standard-normal descriptors, n = %d, C = %d, %2d classes: map(device order) = %.17g, map(float64 order) = %.17g, "
                        "difference = %+.3e; queries whose order differs from float64's: %d" % (n, C, classes, map_dev, map_64, diff, swapped))
    print("\n" + _ERRORS[classes])
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "retrieval", "errors.txt")
    try:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            f.write("sn_retrieval_metrics against float64 on real-valued descriptors (tests/test_gpu_retrieval.py::test_real_valued;\n"
                    "recorded, not asserted: float32 distances may order near-ties differently from float64)\n")
            f.write("".join(_ERRORS[k] + "\n" for k in sorted(_ERRORS)))
    except OSError:
        pass  # (a read-only checkout: the figures were printed)


@pytest.mark.parametrize("classes", [40, 3])
def test_real_valued(classes):
    from samplenet_amd.evaluation import retrieval_aggregates

    n, C, L = 300, 256, 20
    desc, labels = R.normal_case(n, C, classes)
    got = call(desc, labels, L)
    on_device(got[3], got[4])  # a permutation, ascending in (sorted_dist, index), symmetric
    ap, prec, nrel, od, sd = [g.cpu().numpy() for g in got]
    d32, d64 = R.dist32(desc[0]), R.dist64(desc[0])
    assert np.array_equal(sd[0].view(np.int32), np.take_along_axis(d32, od[0].astype(np.int64), axis=1).view(np.int32))
    g64 = np.take_along_axis(d64, od[0].astype(np.int64), axis=1)
    # C products and C - 1 additions, a difference's rounding counted twice through its square: (C + 2) 2^-24 relative
    assert (np.abs(sd[0].astype(np.float64) - g64) <= (C + 2) * 2.0 ** -24 * g64).all()
    a, p, r = R.scores(od[0], labels, L)  # the float64 formulas on the device's own order
    assert np.array_equal(nrel, r)
    assert np.array_equal(ap[0], a.astype(np.float32), equal_nan=True) and np.array_equal(prec[0], p.astype(np.float32), equal_nan=True)
    ref = R.reference(desc[0], labels, L)
    m_dev, m_64 = retrieval_aggregates(a, p, r)["map"], retrieval_aggregates(ref["ap"], ref["prec"], ref["n_relevant"])["map"]
    _record(classes, n, C, m_dev - m_64, m_dev, m_64, int((od[0] != ref["order"]).any(axis=1).sum()))


@pytest.mark.parametrize("kind", ["duplicates", "normal"])
def test_same_call_twice_gives_equal_bytes(kind):
    desc, labels = R.make_case("duplicates", 3, 1025, 64) if kind == "duplicates" else R.normal_case(300, 256, 5)
    a, b = call(desc, labels, 20), call(desc, labels, 20)
    for u, v, name in zip(a, b, NAMES):
        assert torch.equal(u.view(torch.int32), v.view(torch.int32)), name


def test_ops_retrieval_metrics():
    from samplenet_amd import ops

    desc, labels = R.make_case("duplicates", 3, 65, 33, classes=4)
    d, lab = torch.from_numpy(desc).cuda(), torch.from_numpy(labels).cuda()
    ap, prec, nrel, order, sdist = ops.retrieval_metrics(d, lab.long(), levels=7, return_order=True)
    assert ap.dtype == torch.float32 and prec.dtype == torch.float32 and nrel.dtype == torch.int32 and order.dtype == torch.int32
    assert tuple(ap.shape) == (3, 65) and tuple(prec.shape) == (3, 65, 7) and tuple(order.shape) == (3, 65, 64) and not ap.requires_grad
    against_grid_reference(desc, labels, 7, (ap, prec, nrel, order, sdist))
    three = ops.retrieval_metrics(d, lab, 7)
    assert len(three) == 3 and torch.equal(three[0].view(torch.int32), ap.view(torch.int32)) and torch.equal(three[2], nrel)
    flat = ops.retrieval_metrics(d[1], lab, 7, return_order=True)  # one set as (n, C)
    for got, want in zip(flat, (ap[1], prec[1], nrel, order[1], sdist[1])):
        assert got.shape == want.shape and torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert ops.retrieval_metrics(d, lab)[1].shape[2] == 20
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.retrieval_metrics(d.cpu(), lab.cpu())
    with pytest.raises(ValueError, match="one entry per shape"):
        ops.retrieval_metrics(d, lab[:-1])
    with pytest.raises(ValueError, match="desc must be"):
        ops.retrieval_metrics(d[0, 0], lab)
