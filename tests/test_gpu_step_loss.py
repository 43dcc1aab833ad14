"""The sampler step's fused loss entries (include/samplenet_hip_internal.h) called directly with raw pointers, branch by branch: the
pair scan that leaves partial or atomically combined per-point minima, the loss reduction, the one-launch Chamfer + soft-projection
backward and the scalar tail, against the float32 restatement (indices and distances: bit for bit) and the float64 step reference
(values and gradients: counted bounds) of tests/step_loss_ref.py.  Every output, workspace and scratch buffer is a guarded buffer
(tests/cabi_ref.py: poisoned words inside and on both sides).  Every test prints its largest observed error beside its bound
(`pytest -s`; recorded in profiles/step_loss/errors.txt)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import cabi_ref as R
import step_loss_ref as S
from cabi_ref import BCN, BNC, Guarded

pytestmark = pytest.mark.gpu
I32 = torch.int32

FORWARD_CASES = [(s, r) for s in S.ROWS for r in S.RECIPES]
BACKWARD_CASES = [(s, r, "base") for s, r in FORWARD_CASES] + [(s, "cube", n) for n in S.SCALARS if n != "base" for s in S.SCALAR_ROWS]
REFUSAL_ROWS = list(S.DIRECT)
FC_CASES = [(s, k) for s in S.FC_ROWS for k in S.FC_K]
SURFACE_ROWS = list(S.SURFACE_ROWS)
_fid = lambda c: "-".join(S.row_id(x) if isinstance(x, tuple) else str(x) for x in c)


def _lib():
    from samplenet_amd._lib import check, lib

    return lib, check


def dev(a, dtype=None):
    t = torch.from_numpy(np.array(a, order="C")).cuda()  # (a copy: the shared references are read-only)
    return t if dtype is None else t.to(dtype)


def scalar(v):
    return torch.tensor([float(v)], dtype=torch.float32, device="cuda")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same_bits(what, a, b):
    a, b = _bits(a), _bits(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.argwhere(a != b)
    assert not len(bad), "%s: %d of %d elements differ, first at %s: %r against %r" % (
        what, len(bad), a.size, tuple(bad[0]), a[tuple(bad[0])], b[tuple(bad[0])])


def _report(what, err, bound):
    err, bound = np.asarray(err, dtype=np.float64), np.broadcast_to(np.asarray(bound, dtype=np.float64), np.shape(err))
    if err.size:
        i = np.argmax(err / np.maximum(bound, 1e-300))
        print("STEP_ERR %-58s observed %.3e  bound %.3e  ratio %.3f" % (what, err.flat[i], bound.flat[i], err.flat[i] / max(bound.flat[i], 1e-300)))


def _within(what, got, ref, bound):
    err = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(ref, dtype=np.float64))
    _report(what, err, bound)
    bad = ~(err <= np.broadcast_to(bound, err.shape))
    assert not bad.any(), "%s: %d outside the bound, first at %s: %.9e against %.9e, error %.3e, bound %.3e" % (
        what, bad.sum(), tuple(np.argwhere(bad)[0]), np.asarray(got, dtype=np.float64)[bad].flat[0], np.broadcast_to(ref, err.shape)[bad].flat[0],
        err[bad].flat[0], np.broadcast_to(bound, err.shape)[bad].flat[0])


def _u64(g):
    """A guarded buffer of (..., 2) int32 words as unsigned 64-bit keys."""
    return np.ascontiguousarray(g.numpy()).view(np.uint64)[..., 0]


def _written(o, names=None):
    for k, g in o.items():
        if isinstance(g, Guarded) and (names is None or k in names):
            g.check(k)


class Step:
    """One case on the device: the inputs, and one method per entry that allocates guarded outputs, calls, synchronises."""

    def __init__(self, shape, recipe, scalar_case="base"):
        self.shape, self.recipe = shape, recipe
        self.P, self.Q, self.scan = S.reference(shape, recipe)
        self.sc = S.SCALARS[scalar_case]
        B, N, M, K = shape
        self.G = S.scan_plan(B, N, M)[0]
        self.dP, self.dQ = dev(self.P), dev(self.Q.transpose(0, 2, 1))  # (B,N,3) and (B,3,M), the FC head's layout
        self.dT, self.dg = scalar(self.sc[0]), scalar(self.sc[5])
        self.splits = S.soft_bwd_splits(B, M)

    # ---------------------------------------------------------------------------------------- scans
    def _scan_out(self):
        B, N, M, K = self.shape
        return dict(knn=Guarded((B, M, K), I32), dq=Guarded((B, M)), iq=Guarded((B, M), I32), proj=Guarded((B, M, 3)))

    def scan_partial(self, fc=None, ws_bytes=None):
        lib = _lib()[0]
        B, N, M, K = self.shape
        o = self._scan_out()
        o["ws"] = Guarded((B * max(self.G, 1) * N, 2), I32)
        nbytes = B * self.G * N * 8 if ws_bytes is None else ws_bytes
        if fc is None:
            rc = lib.sn_pairscan_forward_partial(B, N, M, K, self.dP.data_ptr(), BNC, self.dQ.data_ptr(), BCN, o["knn"].ptr(), o["dq"].ptr(),
                                                 o["iq"].ptr(), o["proj"].ptr(), BNC, self.dT.data_ptr(), self.sc[1], o["ws"].ptr(), nbytes, None)
        else:
            o["q"] = Guarded((B, 3, M))
            rc = lib.sn_pairscan_forward_partial_fc(B, N, M, K, self.dP.data_ptr(), BNC, *[t.data_ptr() for t in fc[:5]], fc[5], o["q"].ptr(),
                                                    o["knn"].ptr(), o["dq"].ptr(), o["iq"].ptr(), o["proj"].ptr(), BNC, self.dT.data_ptr(),
                                                    self.sc[1], o["ws"].ptr(), nbytes, None)
        torch.cuda.synchronize()
        return rc, o

    def scan_keys(self, fc=None):
        lib = _lib()[0]
        B, N, M, K = self.shape
        G = max(self.G, 1)
        o = self._scan_out()
        o["keys"] = Guarded((B * N, 2), I32, fill=torch.zeros((B * N, 2), dtype=I32))  # zero on entry
        o["qpart"], o["qmax"] = Guarded((B, G, 2)), Guarded((B, G, 2), I32)
        if fc is None:
            q, fcp, kfc = self.dQ.data_ptr(), [None] * 5, 0
        else:
            o["q"] = Guarded((B, 3, M))
            q, fcp, kfc = o["q"].ptr(), [t.data_ptr() for t in fc[:5]], fc[5]
        rc = lib.sn_pairscan_forward_keys(B, N, M, K, self.dP.data_ptr(), BNC, q, *fcp, kfc, o["knn"].ptr(), o["dq"].ptr(), o["iq"].ptr(),
                                          o["proj"].ptr(), BNC, self.dT.data_ptr(), self.sc[1], o["keys"].ptr(), o["qpart"].ptr(),
                                          o["qmax"].ptr(), None)
        torch.cuda.synchronize()
        return rc, o

    def scan_direct(self):
        """sn_pairscan_forward_ws with complete dist_p / idx_p: on a split row the workspace lets it spread a cloud's queries over
        workgroups and finish the minima in its own second launch; on the others one workgroup scans a cloud (N > 2048: two scans)."""
        lib, check = _lib()
        B, N, M, K = self.shape
        o = self._scan_out()
        o["dp"], o["ip"] = Guarded((B, N)), Guarded((B, N), I32)
        nbytes = lib.sn_pairscan_workspace_bytes(B, N, M)
        o["ws"] = Guarded((max(nbytes // 8, 1), 2), I32)
        check(lib.sn_pairscan_forward_ws(B, N, M, K, self.dP.data_ptr(), BNC, self.dQ.data_ptr(), BCN, o["knn"].ptr(), None, o["dq"].ptr(),
                                         o["iq"].ptr(), o["dp"].ptr(), o["ip"].ptr(), o["proj"].ptr(), BNC, None, self.dT.data_ptr(),
                                         self.sc[1], o["ws"].ptr() if nbytes else None, nbytes, None), "sn_pairscan_forward_ws")
        torch.cuda.synchronize()
        assert o["ws"].guards_intact()
        _written(o, ("knn", "dq", "iq", "proj", "dp", "ip"))
        return o

    # ---------------------------------------------------------------------------------------- loss forward
    def loss_partial(self, o, defer):
        lib, check = _lib()
        B, N, M, K = self.shape
        T, ms, alpha, lmbda, weight, g = self.sc
        o.update(dp=Guarded((B, N)), ip=Guarded((B, N), I32), am=Guarded((B,), I32), part=Guarded((B, 4)), loss=Guarded((2,)))
        check(lib.sn_sampler_step_loss_forward(B, M, N, self.G, o["dq"].ptr(), o["ws"].ptr(), o["proj"].ptr(), self.dT.data_ptr(), alpha, lmbda,
                                               weight, ms, o["dp"].ptr(), o["ip"].ptr(), o["am"].ptr(), o["part"].ptr(), o["loss"].ptr(),
                                               int(defer), None), "sn_sampler_step_loss_forward")
        torch.cuda.synchronize()
        _written(o, ("dp", "ip", "am", "part"))
        return o

    def loss_direct(self, o, defer):
        lib, check = _lib()
        B, N, M, K = self.shape
        T, ms, alpha, lmbda, weight, g = self.sc
        o.update(am=Guarded((B,), I32), part=Guarded((B, 4)), loss=Guarded((2,)))
        check(lib.sn_sampler_step_loss_forward_direct(B, M, N, o["dq"].ptr(), o["dp"].ptr(), o["proj"].ptr(), self.dT.data_ptr(), alpha, lmbda,
                                                      weight, ms, o["am"].ptr(), o["part"].ptr(), o["loss"].ptr(), int(defer), None),
              "sn_sampler_step_loss_forward_direct")
        torch.cuda.synchronize()
        _written(o, ("am", "part"))
        return o

    # ---------------------------------------------------------------------------------------- backward
    def _idx(self):
        s = self.scan
        return dev(s["knn"]), dev(s["iq"]), dev(s["ip"]), dev(s["am"])

    def backward(self, deferred=None):
        """sn_sampler_step_loss_backward on the RESTATEMENT's indices (the scan is held to them by its own test)."""
        lib, check = _lib()
        B, N, M, K = self.shape
        T, ms, alpha, lmbda, weight, g = self.sc
        knn, iq, ip, am = self._idx()
        o = dict(gQ=Guarded((B, 3, M)), gsig=Guarded((B * self.splits,)), gT=Guarded((1,)))
        dpart, dloss = (None, None) if deferred is None else (deferred["part"].ptr(), deferred["loss"].ptr())
        check(lib.sn_sampler_step_loss_backward(B, N, M, K, self.dP.data_ptr(), BNC, self.dQ.data_ptr(), knn.data_ptr(), iq.data_ptr(),
                                                ip.data_ptr(), am.data_ptr(), self.dT.data_ptr(), ms, alpha, lmbda, weight, self.dg.data_ptr(),
                                                o["gQ"].ptr(), o["gsig"].ptr(), o["gT"].ptr(), dpart, dloss, None),
              "sn_sampler_step_loss_backward")
        torch.cuda.synchronize()
        _written(o)
        return o

    def keys_backward(self, k, tail=None, grad_proj=None, grad_sigma=None):
        """sn_sampler_step_loss_keys behind scan_keys() (k: its outputs) on the restatement's kNN / idx_q."""
        lib, check = _lib()
        B, N, M, K = self.shape
        T, ms, alpha, lmbda, weight, g = self.sc
        knn, iq, _, _ = self._idx()
        o = dict(gQ=Guarded((B, 3, M)), gsig=Guarded((B * self.splits,)), gT=Guarded((1,)), dpsum=Guarded((B,)), loss=Guarded((2,)))
        check(lib.sn_sampler_step_loss_keys(B, N, M, K, self.dP.data_ptr(), BNC, self.dQ.data_ptr(), knn.data_ptr(), iq.data_ptr(),
                                            k["keys"].ptr(), k["qpart"].ptr(), k["qmax"].ptr(), self.G, self.dT.data_ptr(), ms, alpha, lmbda,
                                            weight, self.dg.data_ptr(), o["gQ"].ptr(), o["gsig"].ptr(), o["gT"].ptr(), o["dpsum"].ptr(),
                                            o["loss"].ptr(), None, tail, None if grad_proj is None else grad_proj.data_ptr(),
                                            None if grad_sigma is None else grad_sigma.data_ptr()), "sn_sampler_step_loss_keys")
        torch.cuda.synchronize()
        assert all(g_.guards_intact() for g_ in o.values()) and k["keys"].guards_intact()
        _written(o, ("gQ", "gsig", "dpsum"))
        return o

    def two_launches(self, grad_proj=None):
        """The op-by-op route: sn_simplification_loss_backward with the sampled cloud in (B,3,M) layout and the upstream gradient
        fp32(alpha g), and sn_soft_project_backward with an explicit grad_proj (default: the constant fp32(g) / fp32(3 B M))."""
        lib, check = _lib()
        B, N, M, K = self.shape
        T, ms, alpha, lmbda, weight, g = self.sc
        knn, iq, ip, am = self._idx()
        up = scalar(np.float32(alpha) * np.float32(g))
        if grad_proj is None:
            grad_proj = torch.full((B, M, 3), float(np.float32(g) / np.float32(B * 3 * M)), dtype=torch.float32, device="cuda")
        o = dict(cham=Guarded((B, 3, M)), soft=Guarded((B, 3, M)), gsig=Guarded((B * self.splits,)))
        check(lib.sn_simplification_loss_backward(B, M, self.dQ.data_ptr(), N, self.dP.data_ptr(), iq.data_ptr(), ip.data_ptr(), am.data_ptr(),
                                                  weight, up.data_ptr(), o["cham"].ptr(), None, 1, None), "sn_simplification_loss_backward")
        check(lib.sn_soft_project_backward(B, N, M, K, self.dP.data_ptr(), BNC, self.dQ.data_ptr(), BCN, knn.data_ptr(), self.dT.data_ptr(), ms,
                                           grad_proj.data_ptr(), BNC, o["soft"].ptr(), BCN, None, o["gsig"].ptr(), None),
              "sn_soft_project_backward")
        torch.cuda.synchronize()
        _written(o)
        return o


def _np(o, *names):
    return [o[n].numpy().copy() for n in names]


# ================================================================================================ a. the scan products, three routes
@functools.lru_cache(maxsize=None)
def forward_products(shape, recipe):
    """Every route's scan products and immediate loss values as numpy; one device pass per case, shared by the tests of a. and b."""
    st = Step(shape, recipe)
    B, N, M, K = shape
    out = {}
    if st.G > 1:
        rc, p = st.scan_partial()
        assert rc == 0, rc
        _written(p)  # the workspace too: every workgroup publishes N keys
        st.loss_partial(p, 0)
        assert p["loss"].fully_written() and p["loss"].guards_intact()
        out["partial"] = {k: v.numpy().copy() for k, v in p.items() if k != "ws"}
        rc, k = st.scan_keys()
        assert rc == 0, rc
        _written(k)
        out["keys"] = {n: v.numpy().copy() for n, v in k.items() if n not in ("keys", "qmax")}
        out["keys"]["keys"], out["keys"]["qmax"] = _u64(k["keys"]).reshape(B, N), _u64(k["qmax"])
        out["keys"]["dp"], out["keys"]["ip"] = S.decode_inverted(out["keys"]["keys"])
    d = st.scan_direct()
    st.loss_direct(d, 0)
    assert d["loss"].fully_written() and d["loss"].guards_intact()
    out["direct"] = {k: v.numpy().copy() for k, v in d.items() if k != "ws"}
    return out


@pytest.mark.parametrize("shape,recipe", FORWARD_CASES, ids=[_fid(c) for c in FORWARD_CASES])
def test_scan_products_of_the_three_routes(shape, recipe):
    """knn_idx, dist_q, idx_q, dist_p, idx_p, argmax1 bit for bit the float32 restatement on every route; proj within 1e-6 of the
    float64 projection on those indices (the bar test_pairscan_weights_against_fp64_softmax holds the scan to at these scales) and
    bit-identical between the routes; the key table decodes to dist_p / idx_p; qpart added over G meets its counted bound; every qmax
    is its workgroup's first maximum (0 / 0 / key 0 from a workgroup without queries); a second run repeats every bit."""
    B, N, M, K = shape
    P, Q, scan = S.reference(shape, recipe)
    L, lsimp, parts = S.reference_loss(shape, recipe, "base")
    per, proj64 = parts[5], parts[6]
    out = forward_products(shape, recipe)
    tag = "%s %s " % (S.row_id(shape), recipe)
    assert ("partial" in out) == ("keys" in out) == (shape in S.SPLIT)
    for route, o in out.items():
        for name, ref in (("knn", "knn"), ("dq", "dq"), ("iq", "iq"), ("dp", "dp"), ("ip", "ip")):
            _same_bits("%s%s %s" % (tag, route, name), o[name], scan[ref])
        if "am" in o:
            _same_bits(tag + route + " argmax1", o["am"], scan["am"])
        _within(tag + route + " proj", o["proj"], proj64, 1e-6)
        for name in ("knn", "dq", "iq", "proj"):
            _same_bits("%s%s against direct: %s" % (tag, route, name), o[name], out["direct"][name])
    if "keys" in out:
        k = out["keys"]
        bq, bp = S.qpart_bound(shape, per, proj64)
        _within(tag + "qpart sum dist_q", k["qpart"][:, :, 0].astype(np.float64).sum(1), per[:, 0], bq)
        _within(tag + "qpart sum proj", k["qpart"][:, :, 1].astype(np.float64).sum(1), per[:, 3], bp)
        want = S.qmax_expected(shape, scan["dq"])
        assert np.array_equal(k["qmax"], want), np.argwhere(k["qmax"] != want)[:4]
        if shape == S.NO_QUERY_ROW:
            assert not k["qmax"][:, -1].any() and not _bits(k["qpart"][:, -1]).any()
    # a second run, from fresh buffers
    again = forward_products.__wrapped__(shape, recipe)
    for route, o in out.items():
        for name, v in o.items():
            _same_bits("%ssecond run, %s %s" % (tag, route, name), v, again[route][name])


# ================================================================================================ b. the loss values
def loss_bounds(shape, recipe, scalar_case="base", with_proj=True):
    L, lsimp, parts = S.reference_loss(shape, recipe, scalar_case)
    if not with_proj:
        L = L - parts[3]
    return (L, lsimp, parts) + S.loss_bound(shape, S.SCALARS[scalar_case], parts, with_proj)


@pytest.mark.parametrize("shape,recipe", FORWARD_CASES, ids=[_fid(c) for c in FORWARD_CASES])
def test_loss_values_immediate_and_deferred(shape, recipe):
    """loss[0] = L and loss[1] = L_simp of the partial and direct routes against float64 under step_loss_ref.loss_bound (the keys
    entry's loss: test_backward_against_fp64); partial [B][4] = sum dq, max dq, sum dp, sum proj per cloud.  With defer_value the
    forward leaves loss[] poisoned and the backward, handed the partials, writes the very bits of the immediate value."""
    L, lsimp, parts, bL, bS, _ = loss_bounds(shape, recipe)
    tag = "%s %s " % (S.row_id(shape), recipe)
    out = forward_products(shape, recipe)
    for route in ("partial", "direct"):
        if route not in out:
            continue
        o = out[route]
        _within(tag + route + " L", o["loss"][0], L, bL)
        _within(tag + route + " L_simp", o["loss"][1], lsimp, bS)
        _within(tag + route + " partial", o["part"], parts[5], S.partial_bound(shape, parts[5], parts[6]))
        st = Step(shape, recipe)
        if route == "partial":
            rc, p = st.scan_partial()
            assert rc == 0
            st.loss_partial(p, 1)
        else:
            p = st.loss_direct(st.scan_direct(), 1)
        assert p["loss"].untouched(), "the forward wrote loss[] although defer_value was set"
        _same_bits(tag + route + " partial, deferred", p["part"].numpy(), o["part"])
        st.backward(deferred=p)
        assert p["loss"].guards_intact()
        _same_bits(tag + route + " deferred loss", p["loss"].check("deferred loss").cpu().numpy(), o["loss"])


# ================================================================================================ c. the backward
def _check_grads(tag, shape, ref, gQ, gT, scalar_case):
    g = S.SCALARS[scalar_case][5]
    _within(tag + "grad_Q", gQ.transpose(0, 2, 1), ref["cham"] + ref["soft"], S.grad_q_bound(ref))
    _within(tag + "grad_T", gT[0], ref["grad_T"], S.grad_t_bound(ref))
    if scalar_case == "clamped":
        assert _bits(gT)[0] == 0, gT  # exactly +0
    if g == 0.0:
        assert not gQ.any() and not gT.any()  # +-0


@pytest.mark.parametrize("shape,recipe,scalar_case", BACKWARD_CASES, ids=[_fid(c) for c in BACKWARD_CASES])
def test_backward_against_fp64(shape, recipe, scalar_case):
    """grad_Q element by element and grad_T against float64 under the counted bounds, for sn_sampler_step_loss_backward (every row;
    N > 2048 takes its three-launch branch) and sn_sampler_step_loss_keys (split rows).  The bits the code promises: the keys entry
    equals the other entry; both equal fp32(sn_simplification_loss_backward) + fp32(sn_soft_project_backward) of the op-by-op route,
    sigma partials included.  Scratch: gsig_scratch has B * sn_soft_bwd_splits floats, all written; after the keys entry the whole
    key table is zero, dpsum holds the per-cloud sum of dist_p, loss meets b.'s bound."""
    lib = _lib()[0]
    B, N, M, K = shape
    st = Step(shape, recipe, scalar_case)
    assert st.splits == lib.sn_soft_bwd_splits(B, M)
    ref = S.reference_grads(shape, recipe, scalar_case)
    tag = "%s %s %s " % (S.row_id(shape), recipe, scalar_case)
    b = st.backward()
    gQ, gsig, gT = _np(b, "gQ", "gsig", "gT")
    _check_grads(tag + "backward ", shape, ref, gQ, gT, scalar_case)
    two = st.two_launches()
    cham, soft, gsig2 = _np(two, "cham", "soft", "gsig")
    _same_bits(tag + "grad_Q against the two launches", gQ, cham + soft)
    _same_bits(tag + "sigma partials against sn_soft_project_backward", gsig, gsig2)
    _same_bits(tag + "second run grad_Q", _np(st.backward(), "gQ")[0], gQ)
    if shape not in S.SPLIT:
        return
    rc, k = st.scan_keys()
    assert rc == 0
    kb = st.keys_backward(k)
    _written(kb)
    kQ, ksig, kT, dpsum, loss = _np(kb, "gQ", "gsig", "gT", "dpsum", "loss")
    _same_bits(tag + "keys grad_Q against sn_sampler_step_loss_backward", kQ, gQ)
    _same_bits(tag + "keys sigma partials", ksig, gsig)
    _same_bits(tag + "keys grad_T", kT, gT)
    _check_grads(tag + "keys ", shape, ref, kQ, kT, scalar_case)
    assert not k["keys"].numpy().any(), "the key table is not zero again: %d words left" % np.count_nonzero(k["keys"].numpy())
    L, lsimp, parts, bL, bS, _ = loss_bounds(shape, recipe, scalar_case)
    _within(tag + "keys dpsum", dpsum, parts[5][:, 2], S.dpsum_bound(shape, parts[5]))
    _within(tag + "keys L", loss[0], L, bL)
    _within(tag + "keys L_simp", loss[1], lsimp, bS)


# ================================================================================================ d. the options of the keys entry
@pytest.mark.parametrize("shape", S.SCALAR_ROWS + (S.NO_QUERY_ROW,), ids=S.row_id)
def test_keys_entry_options(shape):
    """sn_sampler_step_loss_keys with each optional argument.  grad_proj (standard normal): the loss carries no mean(proj) term, grad_Q is
    the Chamfer part + the soft backward of that grad_proj under the same bounds (and the bits of the two op-by-op launches).
    grad_sigma (-0.8): the direct term of grad_T is grad_sigma d sigma / dT, not lmbda g d sigma / dT.  deferred_tail (a host buffer of
    sn_step_tail_bytes()): grad_Q and the sigma partials keep their bits, grad_T and loss stay poisoned, the key table is unchanged;
    the blob is written within its size and not executed here (sn_conv_stack_backward's part, covered through the engine)."""
    B, N, M, K = shape
    recipe = "surface"
    st = Step(shape, recipe)
    P, Q, scan = S.reference(shape, recipe)
    tag = "%s %s " % (S.row_id(shape), recipe)
    rc, k = st.scan_keys()
    assert rc == 0
    table = k["keys"].numpy().copy()
    base = st.keys_backward(k)
    # grad_proj: a task loss outside the node
    rng = np.random.default_rng(11)
    gp = rng.standard_normal((B, M, 3)).astype(np.float32)
    ref = S.step_grads(P, Q, scan, st.sc, grad_proj=gp)
    rc, k2 = st.scan_keys()
    assert rc == 0
    o = st.keys_backward(k2, grad_proj=dev(gp))
    _written(o)
    gQ, gT, loss = _np(o, "gQ", "gT", "loss")
    _within(tag + "grad_proj: grad_Q", gQ.transpose(0, 2, 1), ref["cham"] + ref["soft"], S.grad_q_bound(ref))
    _within(tag + "grad_proj: grad_T", gT[0], ref["grad_T"], S.grad_t_bound(ref))
    L, lsimp, parts, bL, bS, _ = loss_bounds(shape, recipe, with_proj=False)
    _within(tag + "grad_proj: L carries no mean(proj)", loss[0], L, bL)
    _within(tag + "grad_proj: L_simp", loss[1], lsimp, bS)
    two = st.two_launches(grad_proj=dev(gp))
    _same_bits(tag + "grad_proj: grad_Q against the two launches", gQ, two["cham"].numpy() + two["soft"].numpy())
    # grad_sigma: sigma is an output of the caller's node
    ref = S.step_grads(P, Q, scan, st.sc, grad_sigma=-0.8)
    rc, k3 = st.scan_keys()
    assert rc == 0
    o = st.keys_backward(k3, grad_sigma=scalar(-0.8))
    _within(tag + "grad_sigma: grad_T", o["gT"].check("grad_T").cpu().numpy()[0], ref["grad_T"], S.grad_t_bound(ref))
    _same_bits(tag + "grad_sigma: grad_Q", o["gQ"].numpy(), base["gQ"].numpy())
    assert abs(ref["direct"]) > 100 * S.grad_t_bound(ref)  # the direct term is what the case is about
    # deferred_tail: the tail is described, not run
    lib = _lib()[0]
    nb = lib.sn_step_tail_bytes()
    blob = ctypes.create_string_buffer(nb + 64)
    blob.raw = b"\xa5" * (nb + 64)
    rc, k4 = st.scan_keys()
    assert rc == 0
    o = st.keys_backward(k4, tail=ctypes.cast(blob, ctypes.c_void_p))
    _same_bits(tag + "deferred_tail: grad_Q", o["gQ"].numpy(), base["gQ"].numpy())
    _same_bits(tag + "deferred_tail: sigma partials", o["gsig"].numpy(), base["gsig"].numpy())
    assert o["gT"].untouched() and o["loss"].untouched()
    assert np.array_equal(k4["keys"].numpy(), table), "the key table changed although the tail was deferred"
    assert blob.raw[nb:] == b"\xa5" * 64 and blob.raw[:nb] != b"\xa5" * nb  # written, and within sn_step_tail_bytes()


# ================================================================================================ e. the head inside the scan
@pytest.mark.parametrize("shape,Kfc", FC_CASES, ids=[_fid(c) for c in FC_CASES])
def test_head_inside_the_scan(shape, Kfc):
    """sn_pairscan_forward_partial_fc and sn_pairscan_forward_keys with fc_w: q_out against float64 under test_gpu_skinny.py's ceiling,
    identical bits between the two, every scan product bit-equal to the restatement evaluated ON the q_out the kernel wrote, and proj
    against the float64 projection of that q_out under step_loss_ref.proj_bound (1e-6 + what the float32 distances of queries that
    lie far outside the cloud cost)."""
    B, N, M, K = shape
    st = Step(shape, "cube")
    z, scale, shift, W, bias = S.fc_case(shape, Kfc)
    q64, mag = S.fc_ref(z, scale, shift, W, bias)
    assert 0.2 < (z.astype(np.float64) * scale + shift < 0).mean() < 0.45
    fc = [dev(a) for a in (z, scale, shift, W, bias)] + [Kfc]
    tag = "%s Kfc %d " % (S.row_id(shape), Kfc)
    rc, p = st.scan_partial(fc=fc)
    assert rc == 0
    _written(p)
    st.loss_partial(p, 0)
    rc, k = st.scan_keys(fc=fc)
    assert rc == 0
    _written(k)
    q = p["q"].numpy().copy()
    _within(tag + "q_out", q.reshape(B, 3 * M), q64, S.fc_bound(Kfc, mag))
    _same_bits(tag + "q_out, keys entry", k["q"].numpy(), q)
    scan = S.scan_np32(st.P, q.transpose(0, 2, 1), K)
    kdp, kip = S.decode_inverted(_u64(k["keys"]).reshape(B, N))
    for name, got in (("knn", p["knn"]), ("dq", p["dq"]), ("iq", p["iq"]), ("dp", p["dp"]), ("ip", p["ip"]), ("am", p["am"])):
        _same_bits(tag + "partial_fc " + name, got.numpy(), scan[name])
    for name, got in (("knn", k["knn"].numpy()), ("dq", k["dq"].numpy()), ("iq", k["iq"].numpy()), ("dp", kdp), ("ip", kip)):
        _same_bits(tag + "keys fc " + name, got, scan[name])
    _same_bits(tag + "proj between the entries", k["proj"].numpy(), p["proj"].numpy())
    # ... and the projection of THAT q_out onto those neighbours (two entries of one kernel template would agree on a wrong one too)
    sigma = R.sigma_of(st.sc[0], st.sc[1])
    proj64, w64 = R.soft_project(st.P.copy(), q.transpose(0, 2, 1).copy(), scan["knn"], sigma)
    _within(tag + "proj on q_out", p["proj"].numpy(), proj64, S.proj_bound(st.P, q.transpose(0, 2, 1), scan["knn"], sigma, proj64, w64))
    assert np.array_equal(_u64(k["qmax"]), S.qmax_expected(shape, scan["dq"]))


# ================================================================================================ f. the surface pair
@pytest.mark.parametrize("shape", SURFACE_ROWS, ids=S.row_id)
def test_surface_values_behind_a_keys_scan(shape):
    """sn_surface_values_keys right behind a keys scan, with and without simp_bnc: values[0] = L_simp and [2..4] = the three means under
    b.'s bounds, values[1] the bits of sigma_of, simp_bnc the exact transpose of y, the key table read and NOT reset, dpsum and L_simp the
    bits sn_sampler_step_loss_keys leaves afterwards (the kernel comment promises the same order)."""
    lib, check = _lib()
    B, N, M, K = shape
    recipe = "cube"
    st = Step(shape, recipe)
    T, ms, alpha, lmbda, weight, g = st.sc
    L, lsimp, parts, bL, bS, means = loss_bounds(shape, recipe)
    tag = "%s surface values " % S.row_id(shape)
    rc, k = st.scan_keys()
    assert rc == 0
    table = k["keys"].numpy().copy()
    got = {}
    for with_simp in (False, True):
        o = dict(dpsum=Guarded((B,)), values=Guarded((5,)), simp=Guarded((B, M, 3)))
        check(lib.sn_surface_values_keys(B, N, M, st.G, k["keys"].ptr(), k["qpart"].ptr(), k["qmax"].ptr(), st.dT.data_ptr(), ms, weight,
                                         st.dQ.data_ptr() if with_simp else None, o["simp"].ptr() if with_simp else None, o["dpsum"].ptr(),
                                         o["values"].ptr(), None), "sn_surface_values_keys")
        torch.cuda.synchronize()
        _written(o, ("dpsum", "values") + (("simp",) if with_simp else ()))
        assert with_simp or o["simp"].untouched()
        assert np.array_equal(k["keys"].numpy(), table), "the key table is read, not reset"
        v = o["values"].numpy().copy()
        _within(tag + "L_simp", v[0], lsimp, bS)
        assert _bits(v)[1] == _bits(np.float32(R.sigma_of(T, ms)).reshape(1))[0]
        _within(tag + "the three means", v[2:], np.array(parts[:3]), np.array(means))
        got[with_simp] = (v, o["dpsum"].numpy().copy())
        if with_simp:
            _same_bits(tag + "simp_bnc", o["simp"].numpy(), st.Q)
    _same_bits(tag + "both forms, values", got[False][0], got[True][0])
    _same_bits(tag + "both forms, dpsum", got[False][1], got[True][1])
    kb = st.keys_backward(k)
    _same_bits(tag + "dpsum against sn_sampler_step_loss_keys", got[True][1], kb["dpsum"].numpy())
    _same_bits(tag + "L_simp against sn_sampler_step_loss_keys", got[True][0][:1], kb["loss"].check("loss").cpu().numpy()[1:])


@pytest.mark.parametrize("nproj", S.GATHER_SIZES)
def test_surface_gather_upstream(nproj):
    """Exact copies of the three upstream gradients, zeros for each one passed as NULL in turn, guards intact; nproj below, at and above
    one workgroup of 256 and at the headline's 32 x 64 x 3."""
    lib, check = _lib()
    rng = np.random.default_rng(nproj)
    gl, gs, gp = (rng.standard_normal(n).astype(np.float32) for n in (1, 1, nproj))
    for drop in (None, 0, 1, 2):
        ins = [None if i == drop else dev(a) for i, a in enumerate((gl, gs, gp))]
        sc, out = Guarded((2,)), Guarded((nproj,))
        check(lib.sn_surface_gather_upstream(nproj, *[R.arg(t) for t in ins], sc.ptr(), out.ptr(), None), "sn_surface_gather_upstream")
        torch.cuda.synchronize()
        _same_bits("scalars", sc.check("scalars").cpu().numpy(), np.array([0.0 if drop == 0 else gl[0], 0.0 if drop == 1 else gs[0]], np.float32))
        _same_bits("proj_out", out.check("proj_out").cpu().numpy(), np.zeros(nproj, np.float32) if drop == 2 else gp)


# ================================================================================================ g. the scalar entries
@pytest.mark.parametrize("nproj", S.SCALAR_SIZES)
def test_sampler_loss_scalar_entries(nproj):
    """sn_sampler_loss_forward against float64: the 1024-thread sum of proj passes ceil(nproj / 1024) - 1 + 10 additions over any term,
    the quotient, alpha L_simp and lmbda sigma round once each, the two closing additions twice over any term (+ 1 unit of slack).
    sn_sampler_loss_backward: grad_proj = fp32(g / nproj) in every element, grad_lsimp = fp32(alpha g), grad_T by the sigma rule."""
    lib, check = _lib()
    rng = np.random.default_rng(nproj)
    proj = rng.standard_normal(nproj).astype(np.float32)
    lsimp = np.float32(0.37)
    for name in ("base", "clamped", "tie", "negative_g"):
        T, ms, alpha, lmbda, weight, g = S.SCALARS[name]
        a32, l32, g32, T32 = np.float32(alpha), np.float32(lmbda), np.float32(g), np.float32(T)
        sigma = R.sigma_of(T, ms)
        loss = Guarded((1,))
        dproj, dls, dT, dg = dev(proj), scalar(lsimp), scalar(T), scalar(g)
        check(lib.sn_sampler_loss_forward(nproj, dproj.data_ptr(), dls.data_ptr(), dT.data_ptr(), alpha, lmbda, ms, loss.ptr(), None),
              "sn_sampler_loss_forward")
        torch.cuda.synchronize()
        terms = abs(float(a32) * float(lsimp)) + abs(float(l32) * sigma)
        mp = np.abs(proj.astype(np.float64)).sum() / nproj
        bound = S.U * ((max(0, (nproj + 1023) // 1024 - 1) + 10 + 1 + 1) * mp + terms + 2 * (terms + mp))
        _within("nproj %d %s: sn_sampler_loss_forward" % (nproj, name), loss.check("loss").cpu().numpy()[0],
                float(a32) * float(lsimp) + float(l32) * sigma + proj.astype(np.float64).mean(), bound)
        gp, gls, gT = Guarded((nproj,)), Guarded((1,)), Guarded((1,))
        check(lib.sn_sampler_loss_backward(nproj, dg.data_ptr(), dT.data_ptr(), alpha, lmbda, ms, gp.ptr(), gls.ptr(), gT.ptr(), None),
              "sn_sampler_loss_backward")
        torch.cuda.synchronize()
        _same_bits("grad_proj", gp.check("grad_proj").cpu().numpy(), np.full(nproj, g32 / np.float32(nproj), np.float32))
        _same_bits("grad_lsimp", gls.check("grad_lsimp").cpu().numpy(), np.array([a32 * g32], np.float32))
        f = S.sigma_factor(T, ms)
        want = float(l32) * float(g32) * f * 2.0 * float(T32)
        _within("nproj %d %s: grad_T" % (nproj, name), gT.check("grad_T").cpu().numpy()[0], want, 4 * S.U * abs(want))
        assert f != 0.0 or _bits(gT.numpy())[0] == 0


def test_sigma_forward_at_its_three_cases():
    """sigma = max(T^2, min_sigma) with the bits of cabi_ref.sigma_of: T^2 above, below and exactly at min_sigma."""
    lib, check = _lib()
    for name in ("base", "clamped", "tie"):
        T, ms = S.SCALARS[name][:2]
        out, dT = Guarded((1,)), scalar(T)
        check(lib.sn_sigma_forward(dT.data_ptr(), ms, out.ptr(), None), "sn_sigma_forward")
        torch.cuda.synchronize()
        _same_bits("sigma " + name, out.check("sigma").cpu().numpy(), np.array([R.sigma_of(T, ms)], np.float32))


# ================================================================================================ h. refusals that need no device work
@pytest.mark.parametrize("shape", REFUSAL_ROWS, ids=S.row_id)
def test_split_only_entries_refuse_one_workgroup_shapes(shape):
    """On every G <= 1 row sn_pairscan_forward_partial / _partial_fc / _keys (with and without fc_w) answer SN_ERR_UNSUPPORTED and write
    nothing; on the N > 2048 row so does sn_sampler_step_loss_keys."""
    lib = _lib()[0]
    B, N, M, K = shape
    assert lib.sn_pairscan_colmin_splits(B, N, M) == 1
    st = Step(shape, "cube")
    fc = [dev(a) for a in S.fc_case(shape, 8)] + [8]
    for what, (rc, o) in (("partial", st.scan_partial(ws_bytes=1 << 30)), ("partial_fc", st.scan_partial(fc=fc, ws_bytes=1 << 30)),
                          ("keys", st.scan_keys()), ("keys fc", st.scan_keys(fc=fc))):
        assert rc == R.UNSUPPORTED, (what, rc)
        assert b"one workgroup per cloud" in lib.sn_last_error_string()
        for name, g in o.items():
            if name == "keys":
                assert g.guards_intact() and not g.numpy().any(), what
            else:
                assert g.untouched(), (what, name)
    if N > 2048:  # the keys entry itself: N <= 2048
        knn, iq, _, _ = st._idx()
        k = dict(keys=Guarded((B * N, 2), I32), qpart=Guarded((B, 1, 2)), qmax=Guarded((B, 1, 2), I32))
        o = dict(gQ=Guarded((B, 3, M)), gsig=Guarded((B * st.splits,)), gT=Guarded((1,)), dpsum=Guarded((B,)), loss=Guarded((2,)))
        T, ms, alpha, lmbda, weight, g = st.sc
        rc = lib.sn_sampler_step_loss_keys(B, N, M, K, st.dP.data_ptr(), BNC, st.dQ.data_ptr(), knn.data_ptr(), iq.data_ptr(), k["keys"].ptr(),
                                           k["qpart"].ptr(), k["qmax"].ptr(), 1, st.dT.data_ptr(), ms, alpha, lmbda, weight, st.dg.data_ptr(),
                                           o["gQ"].ptr(), o["gsig"].ptr(), o["gT"].ptr(), o["dpsum"].ptr(), o["loss"].ptr(), None, None, None,
                                           None)
        torch.cuda.synchronize()
        assert rc == R.UNSUPPORTED and b"N <= 2048" in lib.sn_last_error_string()
        assert all(g_.untouched() for g_ in list(k.values()) + list(o.values()))


def test_partial_workspace_one_byte_short():
    """A partial-scan workspace one byte below B G N 8 is SN_ERR_BAD_ARGUMENT before any device work; exactly that size is served."""
    lib = _lib()[0]
    shape = (2, 64, 33, 8)
    st = Step(shape, "cube")
    fc = [dev(a) for a in S.fc_case(shape, 8)] + [8]
    for f in (None, fc):
        rc, o = st.scan_partial(fc=f, ws_bytes=S.partial_ws_bytes(shape) - 1)
        assert rc == R.BAD_ARGUMENT and b"workspace too small" in lib.sn_last_error_string()
        assert all(g.untouched() for g in o.values())
        rc, o = st.scan_partial(fc=f, ws_bytes=S.partial_ws_bytes(shape))
        assert rc == 0


# ================================================================================================ i. the Python hand-off
HANDOFF_CASES = [((2, 64, 33, 8), "partial"), ((2, 64, 33, 8), "keys"), ((3, 64, 16, 8), "direct"), ((2, 2112, 5, 8), "direct")]


@pytest.mark.parametrize("shape,route", HANDOFF_CASES, ids=[_fid(c) for c in HANDOFF_CASES])
def test_python_hand_off_equals_the_entries(shape, route):
    """ops.step_loss_forward -> ops.step_loss_backward through the StepLossState record on the smallest row of each route (partial key
    sets; the keys route on a caller's zeroed table; one workgroup per cloud; N > 2048 with its three-launch backward), the loss value
    immediate and deferred: proj, the loss, grad_Q and grad_T carry the BITS this file's harness gets from the C entries called directly
    on the same inputs -- the same kernels with the same arguments, so anything else is a wiring error.  The record's fields are None
    exactly where the route does not produce them, the key table is zero again behind the keys-mode backward, and without a
    deferred tail there is nothing to keep."""
    from samplenet_amd import ops

    B, N, M, K = shape
    st = Step(shape, "surface")
    T, ms, alpha, lmbda, weight, g = st.sc
    cfg = ops.StepCfg(K, ms, alpha, lmbda, weight)
    assert cfg == (K, ms, alpha, lmbda, weight) and cfg.weight == weight
    assert (ops.scan_splits(B, N, M) > 1) == (route != "direct") and ops.scan_splits(B, N, M) == max(st.G, 1)
    for defer in ((True,) if route == "keys" else (False, True)):
        tag = "%s %s defer=%d " % (S.row_id(shape), route, defer)
        if route == "keys":
            rc, e = st.scan_keys()
            assert rc == 0
            b = st.keys_backward(e)
            loss_e = b["loss"]
        else:
            if route == "partial":
                rc, e = st.scan_partial()
                assert rc == 0
                st.loss_partial(e, defer)
            else:
                e = st.scan_direct()
                st.loss_direct(e, defer)
            b = st.backward(e if defer else None)
            loss_e = e["loss"]
        keys = torch.zeros(B * N, dtype=torch.int64, device="cuda") if route == "keys" else None
        loss, proj, state = ops.step_loss_forward(st.dP, st.dQ, None, st.dT, K, ms, alpha, lmbda, weight, defer, keys=keys)
        gQ, gT, keep = ops.step_loss_backward(st.dP, st.dQ, st.dT, state, cfg, st.dg, None)
        torch.cuda.synchronize()
        _same_bits(tag + "proj", proj.cpu().numpy(), e["proj"].numpy())
        _same_bits(tag + "loss", loss.cpu().numpy(), loss_e.check("loss").cpu().numpy())
        _same_bits(tag + "grad_Q", gQ.cpu().numpy(), b["gQ"].numpy())
        _same_bits(tag + "grad_T", gT.cpu().numpy(), b["gT"].check("grad_T").cpu().numpy())
        assert keep is None
        _same_bits(tag + "state.idx", state.idx.cpu().numpy(), e["knn"].numpy())
        _same_bits(tag + "state.idx_q", state.idx_q.cpu().numpy(), e["iq"].numpy())
        if route == "keys":
            assert state.keys_mode and state.keys is keys and state.G == st.G
            assert state.idx_p is None and state.argmax1 is None
            assert state.qpart.shape == (B * st.G * 2,) and state.qmax.shape == (B * st.G,)
            assert state.deferred[0] is not None and state.deferred[1] is loss
            assert not keys.any().item(), "the key table is not zero again"
        else:
            assert not state.keys_mode
            assert state.keys is None and state.qpart is None and state.qmax is None and state.G is None
            _same_bits(tag + "state.idx_p", state.idx_p.cpu().numpy(), e["ip"].numpy())
            _same_bits(tag + "state.argmax1", state.argmax1.cpu().numpy(), e["am"].numpy())
            if defer:
                assert state.deferred[0] is not None and state.deferred[1] is loss
            else:
                assert state.deferred == (None, None)
