"""Host-side half of the direct step-loss tests (no GPU): tests/step_loss_ref.py is honest -- every row's G and sigma-partial count are
what the library's host functions answer, the "no query" row really leaves a scan workgroup empty, the partial-scan workspace has the
documented size, the float32 restatement of the scan agrees bit for bit with the C oracle on every row and recipe, the float64 step
reference agrees with central differences of its own loss, the sigma rule holds at its three cases -- and tests/test_gpu_step_loss.py
reaches every entry and every row of the table."""
import os
import re

import numpy as np
import pytest

import cabi_ref as R
import step_loss_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from built_lib import ensure_built

    ensure_built()
    from samplenet_amd._lib import lib as L

    return L


def test_every_row_has_the_splits_the_library_answers(lib):
    assert len(set(S.ROWS)) == len(S.ROWS) == 14
    for shape, G, why in S.SPLIT_ROWS:
        B, N, M, K = shape
        assert lib.sn_pairscan_colmin_splits(B, N, M) == G == S.scan_plan(B, N, M)[0] > 1, (shape, why)
    for shape, why in S.DIRECT_ROWS:
        B, N, M, K = shape
        assert lib.sn_pairscan_colmin_splits(B, N, M) == S.scan_plan(B, N, M)[0] == 1, (shape, why)
    for B, N, M, K in S.ROWS:
        assert lib.sn_soft_bwd_splits(B, M) == S.soft_bwd_splits(B, M), (B, M)
        assert B * N * M <= S.MAX_PAIRS and 1 <= K <= min(N, 64)
    assert lib.sn_pairscan_colmin_splits(0, 8, 8) == 0 and lib.sn_pairscan_colmin_splits(2, 0, 8) == 0 and lib.sn_pairscan_colmin_splits(2, 8, -1) == 0


def test_route_functions_answer_the_table(lib):
    """ops.scan_splits / ops.keys_step_possible, which every Python caller of the chain decides its route by: the table's G on every
    row, the keys-mode step exactly on the split rows (all of them N <= 2048; (2, 2112, 5, 8) stands on the other side of that
    bound), and on none with the test hook off."""
    from samplenet_amd import fused_step, ops

    assert any(s[1] > 2048 for s in S.DIRECT) and all(s[1] <= 2048 for s in S.SPLIT)
    for shape, G, why in S.SPLIT_ROWS:
        B, N, M, K = shape
        assert ops.scan_splits(B, N, M) == G, (shape, why)
        assert ops.keys_step_possible(B, N, M) is True, (shape, why)
    for shape, why in S.DIRECT_ROWS:
        B, N, M, K = shape
        assert ops.scan_splits(B, N, M) == 1, (shape, why)
        assert ops.keys_step_possible(B, N, M) is False, (shape, why)
    old = fused_step.KEYS_LOSS
    try:
        fused_step.KEYS_LOSS = False
        assert not any(ops.keys_step_possible(*s[:3]) for s in S.ROWS)
    finally:
        fused_step.KEYS_LOSS = old


def test_rows_reach_the_branches_they_are_named_for():
    plan = {s: S.scan_plan(*s[:3]) for s in S.ROWS}
    B, N, M, K = S.NO_QUERY_ROW
    G, qpb, waves = plan[S.NO_QUERY_ROW]
    assert (G, qpb) == (6, 5) and (G - 1) * qpb >= M > (G - 2) * qpb  # workgroup 5 starts at query 25 = M: it scans nothing
    assert B > 64
    assert plan[(2, 1100, 9, 8)][2] == 3 and plan[(512, 64, 17, 4)] == (1, 17, 4) and plan[(3, 64, 16, 8)] == (1, 16, 16)
    # points per lane of the scan and of chamfer_soft_bwd_kernel: 1 / 4 / 16 / 32 and the edges 64 / 256 / 1024 / 2048
    ns = {s[1] for s in S.ROWS}
    assert {1, 64, 200, 256, 1000, 1024, 1100, 2048, 2112} <= ns
    # the threshold's lane groups: K = 1 (LOGG 0), <= 8 (3), <= 16 (4), > 16 (6) -- all among the SPLIT rows, where qpart is produced
    ks = {s[3] for s in S.SPLIT}
    assert 1 in ks and ks & {2, 3, 4, 5, 6, 7, 8} and 16 in ks and 17 in ks and 64 in ks
    assert all(s in S.SPLIT for s in S.FC_ROWS + S.SURFACE_ROWS + S.SCALAR_ROWS) and any(s[0] > 64 for s in S.SURFACE_ROWS)


def test_partial_workspace_is_B_G_N_keys(lib):
    for shape, G, _ in S.SPLIT_ROWS:
        B, N, M, K = shape
        assert S.partial_ws_bytes(shape) == B * lib.sn_pairscan_colmin_splits(B, N, M) * N * 8


CASES = [(s, r) for s in S.ROWS for r in S.RECIPES]


@pytest.mark.parametrize("shape,recipe", CASES, ids=["%s-%s" % (S.row_id(s), r) for s, r in CASES])
def test_restatement_agrees_with_the_c_oracle(oracle, shape, recipe):
    P, Q, scan = S.reference(shape, recipe)
    od, oi = oracle.knn(shape[3], P, Q)
    assert np.array_equal(oi, scan["knn"])
    assert np.array_equal(od[:, :, 0].view(np.int32), scan["dq"].view(np.int32))
    d1, i1, d2, i2 = oracle.chamfer_forward(Q, P)
    assert np.array_equal(d1.view(np.int32), scan["dq"].view(np.int32)) and np.array_equal(i1, scan["iq"])
    assert np.array_equal(d2.view(np.int32), scan["dp"].view(np.int32)) and np.array_equal(i2, scan["ip"])
    assert np.array_equal(scan["am"], scan["dq"].argmax(1))
    if recipe == "on_points":
        assert not scan["dq"].any() and not scan["am"].any()
    if recipe == "coincident":
        assert not scan["ip"].any()
    if recipe == "cube" and shape[1] >= 8 and shape[1] // 2 >= 4:
        n = shape[1] // 2
        assert np.array_equal(scan["dp"][:, n:n + 4].view(np.int32), scan["dp"][:, 0:4].view(np.int32))


def test_step_reference_against_central_differences():
    shape, sc = (1, 5, 3, 2), (0.6, 1e-2, 0.3, 0.7, 1.64, 1.0)
    rng = np.random.default_rng(5)
    P = (rng.random((1, 5, 3)) - 0.5).astype(np.float32)
    Q = (rng.random((1, 3, 3)) - 0.5).astype(np.float32)
    scan = S.scan_np32(P, Q, 2)
    ref = S.step_grads(P, Q, scan, sc)
    gQ = ref["cham"] + ref["soft"]
    h = 1e-6
    Q64 = Q.astype(np.float64)
    for j in range(3):
        for c in range(3):
            qp, qm = Q64.copy(), Q64.copy()
            qp[0, j, c] += h
            qm[0, j, c] -= h
            fd = (S.step_loss(P, qp, scan, sc)[0] - S.step_loss(P, qm, scan, sc)[0]) / (2 * h)
            assert abs(fd - gQ[0, j, c]) <= 1e-7 * abs(fd), (j, c, fd, gQ[0, j, c])
    # temperature: L through sigma = T^2 (T^2 > min_sigma here), in float64 around the float32 T
    T = float(np.float32(sc[0]))

    def L_of(t):
        lsimp = S.step_loss(P, Q, scan, sc)[1]
        proj, _ = R.soft_project(P, Q, scan["knn"], t * t)  # (sigma = T^2 in float64; the step's sigma is its float32 value, 6e-8 away)
        return float(np.float32(sc[2])) * lsimp + float(np.float32(sc[3])) * t * t + proj.mean()

    fd = (L_of(T + h) - L_of(T - h)) / (2 * h)
    assert abs(fd - ref["grad_T"]) <= 1e-7 * abs(fd), (fd, ref["grad_T"])
    assert ref["grad_T_abs"] >= abs(ref["grad_T"])


def test_sigma_rule_at_its_three_cases():
    for name, want in (("base", 1.0), ("clamped", 0.0), ("tie", 0.5)):
        T, ms = S.SCALARS[name][:2]
        assert S.sigma_factor(T, ms) == want
        assert R.sigma_of(T, ms) == (float(np.float32(T) * np.float32(T)) if want else float(np.float32(ms)))
    T, ms = S.SCALARS["tie"][:2]
    assert np.float32(T) * np.float32(T) == np.float32(ms)
    rng = np.random.default_rng(1)
    P, Q = (rng.random((1, 6, 3)) - 0.5).astype(np.float32), (rng.random((1, 2, 3)) - 0.5).astype(np.float32)
    scan = S.scan_np32(P, Q, 3)
    full = S.step_grads(P, Q, scan, S.SCALARS["base"])
    for name, want in (("clamped", 0.0), ("tie", 0.5)):
        ref = S.step_grads(P, Q, scan, S.SCALARS[name])
        T = float(np.float32(S.SCALARS[name][0]))
        assert ref["grad_T"] == ref["sig_terms"].sum() * 2 * T * want + ref["direct"]
        assert ref["direct"] == float(np.float32(0.7)) * 1.0 * 2 * T * want
    assert full["direct"] == float(np.float32(0.7)) * 2 * float(np.float32(0.6))
    gs = S.step_grads(P, Q, scan, S.SCALARS["base"], grad_sigma=-0.8)
    assert gs["direct"] == float(np.float32(-0.8)) * 2 * float(np.float32(0.6))


ENTRIES = ("sn_pairscan_colmin_splits", "sn_pairscan_forward_partial", "sn_pairscan_forward_partial_fc", "sn_pairscan_forward_keys",
           "sn_pairscan_forward_ws", "sn_sampler_step_loss_forward", "sn_sampler_step_loss_forward_direct",
           "sn_sampler_step_loss_backward", "sn_sampler_step_loss_keys", "sn_surface_values_keys", "sn_surface_gather_upstream",
           "sn_sampler_loss_forward", "sn_sampler_loss_backward", "sn_sigma_forward", "sn_simplification_loss_backward",
           "sn_soft_project_backward", "sn_soft_bwd_splits", "sn_step_tail_bytes")


def test_the_gpu_file_reaches_every_entry_and_every_row():
    """So that the list cannot rot: every entry of the step-loss family is called by tests/test_gpu_step_loss.py (as lib.sn_*), the
    argument table of tests/test_cabi_arguments.py holds the twelve entries the family adds to it, and the tests that walk the table
    are parametrised over ALL of its rows, recipes and scalar cases."""
    with open(os.path.join(ROOT, "tests", "test_gpu_step_loss.py")) as f:
        text = f.read()
    called = set(re.findall(r"lib\.(sn_[a-z0-9_]+)", text))
    assert not set(ENTRIES) - called, set(ENTRIES) - called
    import test_cabi_arguments as A
    import test_gpu_step_loss as G

    assert set(A.STEP_LOSS) == {"sn_pairscan_forward_partial", "sn_pairscan_forward_partial_fc", "sn_pairscan_forward_keys",
                                "sn_sampler_step_loss_forward", "sn_sampler_step_loss_forward_direct", "sn_sampler_step_loss_backward",
                                "sn_sampler_step_loss_keys", "sn_surface_values_keys", "sn_surface_gather_upstream",
                                "sn_sampler_loss_forward", "sn_sampler_loss_backward", "sn_sigma_forward"}
    assert set(G.FORWARD_CASES) == {(s, r) for s in S.ROWS for r in S.RECIPES}
    assert {c[:2] for c in G.BACKWARD_CASES if c[2] == "base"} == set(G.FORWARD_CASES)
    for name in S.SCALARS:
        assert len({c[0] for c in G.BACKWARD_CASES if c[2] == name}) >= 2, name
    assert set(G.REFUSAL_ROWS) == set(S.DIRECT) and set(G.FC_CASES) == {(s, k) for s in S.FC_ROWS for k in S.FC_K}
    assert set(G.SURFACE_ROWS) == set(S.SURFACE_ROWS)
