"""The skinny FC entries and sn_bn_relu_*, called directly, shape by shape.

sn_skinny_linear / sn_skinny_linear2 / sn_skinny_wgrad (csrc/task_network.hip) carry the autoencoder's decoder, the classifier's FC heads
and PCRNet's trunk; sn_bn_relu_* (csrc/cloud_transform.hip) sit between the classifier heads' layers.  The network tests reach them
only at the networks' own widths and judge six layers at once by a maximum or a norm.  Here every branch of the kernels gets a shape of
its own (tests/skinny_ref.py: PLANS) and every element is compared: integer data bit for bit against the fp64 reference, real data
element by element against the component-wise magnitude A = |x| |W|^T + |b|.  Every output, the slice scratch and the arrival
counters are views into sentinel-filled buffers (the helper's check() asserts that nothing outside a view changed and that the counters
are back at zero), so an out-of-range row or column is a failed assertion here, never a fault."""
import itertools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import skinny_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu

# Worst |F.linear in fp32 - fp64| / A of torch's own fp32 route over the data of test_real_data_element_by_element, per K class
# (K <= 64, <= 1024, > 1024): tools/skinny_floors.py measures them (python tools/skinny_floors.py > profiles/skinny/floors.txt) and
# the bar is 4 x these.  NOT MEASURED YET (None): until the three figures of that file's last lines are copied here, the test stands
# on its hard ceiling (K + 8) 2^-24 alone.
TORCH_FP32_FLOOR = (None, None, None)
MARGIN = 4.0

_ids = lambda kn: "K%d-N%d" % kn


def _layouts(W):
    return ((0, W), (1, W.t().contiguous()))


def _exact(got, ref):
    return got is not None and torch.equal(got.double(), ref)


@pytest.mark.parametrize("shape", S.SHAPES, ids=_ids)
def test_plan_and_scratch_size(shape):
    """The plan is asserted through its one visible consequence: scratch bytes = S slices x 32-column tiles x row tiles x 4096."""
    from samplenet_amd._lib import lib

    K, N = shape
    slices, _ = S.PLANS[shape]
    for R in S.ROWS_FULL:
        assert lib.sn_skinny_linear_supported(R, K, N) and lib.sn_skinny_linear_supported(R, N, K)
        assert lib.sn_skinny_linear_scratch_bytes(R, K, N) == slices * ((N + 31) // 32) * S.row_tiles(R) * 4096, (R, K, N)


@pytest.mark.parametrize("shape", S.SHAPES, ids=_ids)
def test_integers_bit_exact(shape):
    """(a) single-plane integers: every combination of gate, relu and bias, both layouts, every row count of the shape, against the
    fp64 reference with torch.equal.  The gate holds zeros and negatives: `> 0` is told from `>= 0` and `!= 0`."""
    K, N = shape
    for R in S.rows_of(shape):
        x, gate, W, bias = S.integer_case(R * 131 + K * 7 + N, R, K, N)
        assert R * K == 1 or (bool((gate == 0).any()) and bool((gate < 0).any()))
        for use_gate, relu, use_bias in itertools.product((False, True), repeat=3):
            ref, A = S.linear_ref(x, None, gate if use_gate else None, W, False, bias if use_bias else None, relu)
            assert float(A.max()) < 2 ** 17
            for tr, Wl in _layouts(W):
                c = S.launch_linear(x, Wl, tr, gate=gate if use_gate else None, bias=bias if use_bias else None, relu=relu).check()
                assert _exact(c.out, ref), (c.what, float((c.out.double() - ref).abs().max()))


def _three_plane(g, rows, K):
    """Quarter-integers m / 4 with |m| < 2^19 (|value| < 2^17): 19 significant bits, so the third bf16 plane is not zero."""
    return torch.randint(-2 ** 19 + 1, 2 ** 19, (rows, K), device="cuda", generator=g).float() / 4


def _two_plane(g, shape):
    """Three in four values odd with 257 <= |v| <= 1023 (nine or ten significant bits: no bf16 holds them), the rest in [-4, 4]."""
    big = (torch.randint(128, 512, shape, device="cuda", generator=g) * 2 + 1).float()
    sign = torch.randint(0, 2, shape, device="cuda", generator=g).float() * 2 - 1
    small = torch.randint(-4, 5, shape, device="cuda", generator=g).float()
    return torch.where(torch.rand(shape, device="cuda", generator=g) < 0.75, big * sign, small)


@pytest.mark.parametrize("case", ("x3", "W3", "x2W2"))
@pytest.mark.parametrize("shape", ((7, 5), (8, 32), (32, 33)), ids=_ids)
def test_multi_plane_products_bit_exact(shape, case):
    """(a) a dropped or duplicated product of the three-way bf16 split.  x3: x needs all three planes, W one (|W| <= 3, five non-zeros
    per column): terms (0,0), (1,0), (2,0).  W3: the mirror image, (0,1) and (0,2).  x2W2: both operands need two planes (|v| < 2^10,
    eight non-zero k per row of x): (1,1).  The three-plane operand is a quarter-integer with |m| < 2^19, not an integer: every integer
    below 2^17 is already exact in TWO planes (the residual of an 8-bit rounding at 2^16 is at most 256), and the third plane is the
    point; |x| < 2^17, |W| <= 3 and sum_k |x| |W| < 2^23 hold as stated, and with all data multiples of 1/4 and the scaled sums below
    2^23 every partial sum in any order is exact in fp32.  The planes' use is asserted on the inputs."""
    K, N = shape
    g = S.gen(K * 1009 + N * 13 + len(case))
    small = lambda sh: (torch.randint(1, 4, sh, device="cuda", generator=g) * (torch.randint(0, 2, sh, device="cuda", generator=g) * 2 - 1)).float()
    for R in (5, 33, 128):
        if case == "x3":
            x, W = _three_plane(g, R, K), S.sparse_rows(g, N, K, 5, small)
            assert float((S.split3_ref(x)[2] != 0).float().mean()) > 0.25 and float(x.abs().max()) < 2 ** 17 and float(W.abs().max()) <= 3
        elif case == "W3":
            x, W = S.sparse_rows(g, R, K, 5, small), _three_plane(g, N, K)
            assert float((S.split3_ref(W)[2] != 0).float().mean()) > 0.25 and float(W.abs().max()) < 2 ** 17 and float(x.abs().max()) <= 3
        else:
            x, W = S.sparse_rows(g, R, K, 8, lambda sh: _two_plane(g, sh)), _two_plane(g, (N, K))
            for t in (x[x != 0], W):
                assert float((S.split3_ref(t)[1] != 0).float().mean()) >= 0.5 and float(t.abs().max()) < 2 ** 10
        ref, A = S.linear_ref(x, None, None, W, False, None, False)
        assert float(A.max()) < 2 ** 23
        assert torch.equal(torch.stack(S.split3_ref(x)).double().sum(0), x.double()) and torch.equal(torch.stack(S.split3_ref(W)).double().sum(0), W.double())
        for tr, Wl in _layouts(W):
            c = S.launch_linear(x, Wl, tr).check()
            assert _exact(c.out, ref), (case, c.what, float(((c.out.double() - ref).abs() / A.clamp_min(1)).max()))


@pytest.mark.parametrize("shape", ((72, 40), (584, 70), (1024, 512)), ids=_ids)
def test_two_part_operands_bit_exact(shape):
    """(a) x2 / ksplit and out2 / nsplit: each present half equals the matching column slice of the unsplit result (itself equal to the
    integer reference), with both outputs, `out` NULL and `out2` NULL."""
    K, N = shape
    for R in S.ROWS_FEW:
        x, gate, W, bias = S.integer_case(R * 17 + K + N * 3, R, K, N)
        for tr, Wl in _layouts(W):
            whole = S.launch_linear(x, Wl, tr, bias=bias, relu=True).check().out
            assert _exact(whole, S.linear_ref(x, None, None, W, False, bias, True)[0])
            gated = S.launch_linear(x, Wl, tr, gate=gate).check().out
            assert _exact(gated, S.linear_ref(x, None, gate, W, False, None, False)[0])
            for ksplit in (8, 24, 64, K - 8):
                xa, xb = x[:, :ksplit].contiguous(), x[:, ksplit:].contiguous()
                c = S.launch_linear(xa, Wl, tr, x2=xb, bias=bias, relu=True).check()
                assert torch.equal(c.out, whole), c.what
            for nsplit, want in itertools.product((1, 31, 32, N - 1), ((True, True), (False, True), (True, False))):
                c = S.launch_linear(x, Wl, tr, gate=gate, nsplit=nsplit, want=want).check()
                assert (c.out is not None, c.out2 is not None) == want
                assert not want[0] or torch.equal(c.out, gated[:, :nsplit]), c.what
                assert not want[1] or torch.equal(c.out2, gated[:, nsplit:]), c.what
            # both at once: the trunk's first layer forward has x2, its data gradient the split output
            c = S.launch_linear(x[:, :64].contiguous(), Wl, tr, x2=x[:, 64:].contiguous(), bias=bias, relu=True, nsplit=31).check()
            assert torch.equal(c.out, whole[:, :31]) and torch.equal(c.out2, whole[:, 31:]), c.what


@pytest.mark.parametrize("shape", S.FULL_ROW_SHAPES + ((1600, 3), (2048, 1024)), ids=_ids)
def test_memory_contract(shape):
    """(b) outputs, scratch (exactly sn_skinny_linear_scratch_bytes) and counters between guard words, every row count: no guard word
    changes, the counters return to zero, and every element of every output is written (none still holds the sentinel)."""
    K, N = shape
    for R in S.ROWS_FULL:
        x, gate, W, bias = S.real_case(R + K, R, K, N)
        for tr, Wl in _layouts(W):
            ns = min(31, N - 1)
            for c in (S.launch_linear(x, Wl, tr, gate=gate, bias=bias, relu=True), S.launch_linear(x, Wl, tr, nsplit=ns),
                      S.launch_linear(x, Wl, tr, nsplit=ns, want=(False, True)), S.launch_linear(x, Wl, tr, nsplit=ns, want=(True, False))):
                c.check()
                for gb in c.outs:
                    assert not bool(torch.isnan(gb.view).any()), c.what


def test_shared_scratch_and_repeatability():
    """(c) one (scratch, counters) pair sized as the trunk sizes it (the maximum over its layers, both directions), eight launches back
    to back on one stream with no host synchronisation, twice: every output equals its stand-alone result and the second pass the
    first, bit for bit."""
    from samplenet_amd._lib import lib

    R, shapes = 97, ((2048, 1024), (1024, 512), (576, 33), (1600, 3))
    nbytes = max(max(lib.sn_skinny_linear_scratch_bytes(R, K, N), lib.sn_skinny_linear_scratch_bytes(R, N, K)) for K, N in shapes)
    shared = S.Scratch(nbytes, max((max(K, N) + 31) // 32 for K, N in shapes))
    data = [S.real_case(K + N, R, K, N) for K, N in shapes]
    jobs = [(d, 0, d[2]) for d in data] + [(d, 1, d[2].t().contiguous()) for d in reversed(data)]
    alone = [S.launch_linear(d[0], Wl, tr, gate=d[1], bias=d[3], relu=True).check().out for d, tr, Wl in jobs]
    torch.cuda.synchronize()
    passes = [[S.launch_linear(d[0], Wl, tr, gate=d[1], bias=d[3], relu=True, scratch=shared) for d, tr, Wl in jobs] for _ in range(2)]
    torch.cuda.synchronize()
    for p in passes:
        for c, want in zip(p, alone):
            c.check()
            assert torch.equal(c.out, want), c.what
    for c1, c2 in zip(*passes):
        assert torch.equal(c1.out, c2.out), c1.what


def real_ratios(shape, seeds=(0, 1, 2), rows=S.ROWS_FEW, route="library"):
    """Worst |got - fp64| / A over the data of test (d), for the library's kernel or for torch's F.linear in fp32 (the reference route of
    the measured bar: tools/skinny_floors.py).  -> {(R, variant, layout): ratio}"""
    K, N = shape
    worst = {}
    for seed, R in itertools.product(seeds, rows):
        x, gate, W, bias = S.real_case(seed * 7919 + R * 31 + K + N, R, K, N)
        for variant, (gt, relu) in (("gated-relu", (gate, True)), ("plain", (None, False))):
            ref, A = S.linear_ref(x, None, gt, W, False, bias, relu)
            for tr, Wl in _layouts(W):
                if route == "library":
                    got = S.launch_linear(x, Wl, tr, gate=gt, bias=bias, relu=relu).check().out
                else:
                    xin = x if gt is None else x * (gt > 0).float()
                    got = F.linear(xin, Wl.t() if tr else Wl, bias)
                    got = got.clamp_min(0) if relu else got
                key = (R, variant, tr)
                worst[key] = max(worst.get(key, 0.0), float(((got.double() - ref).abs() / A).max()))
    return worst


@pytest.mark.parametrize("shape", S.SHAPES, ids=_ids)
def test_real_data_element_by_element(shape):
    """(d) standard-normal x, W ~ K^-1/2, a ReLU-output gate, three seeds, R in {5, 33, 128}, both layouts, with gate + bias + relu and
    plain: per element, ratio = |got - fp64| / A (A the pre-activation's magnitude: ReLU is 1-Lipschitz) stays under
      the ceiling (K + 8) 2^-24 -- fp32 accumulation of K terms, the three products the split omits, the epilogue -- and under
      4 x the worst ratio torch's own fp32 F.linear shows on the same data in this K class (TORCH_FP32_FLOOR)."""
    K, N = shape
    worst = real_ratios(shape)
    top, ceiling, floor = max(worst.values()), (K + 8) * 2.0 ** -24, TORCH_FP32_FLOOR[S.k_class(K)]
    print("skinny (%d, %d): worst ratio %.3e  ceiling %.3e  measured bar %s" % (K, N, top, ceiling, "unmeasured" if floor is None else "%.3e" % (MARGIN * floor)))
    for key, r in worst.items():
        assert r <= ceiling, (shape, key, r)
        assert floor is None or r <= MARGIN * floor, (shape, key, r)


WGRAD_SHAPES = ((1, 1), (33, 31), (130, 40), (160, 7), (1024, 64))
WGRAD_ROWS = (1, 2, 5, 33, 128, 129, 255, 256)


@pytest.mark.parametrize("shape", WGRAD_SHAPES, ids=_ids)
def test_wgrad(shape):
    """(e) sn_skinny_wgrad: fp32 MFMAs, products rounded once, rows ascending.  Integers in [-4, 4]: dW and db bit-exact; real data:
    |err| <= (R + 2) 2^-24 of the fp64 magnitude, element by element; gate on / off, db NULL or not, x2 at ksplit in {5, 32, 48,
    K - 1} (a wave straddles the two parts); guard words around dW and db; a second run gives the same bits."""
    K, N = shape
    splits = [None] + sorted({k for k in (5, 32, 48, K - 1) if 0 < k < K})
    for R in WGRAD_ROWS:
        g = S.gen(R * 977 + K * 3 + N)
        xi, dyi, gate = S.ints(g, -4, 4, R, K), S.ints(g, -4, 4, R, N), S.ints(g, -2, 2, R, N)
        xr, dyr = torch.randn(R, K, device="cuda", generator=g), torch.randn(R, N, device="cuda", generator=g)
        for use_gate in (False, True):
            gt = gate if use_gate else None
            for x, dy, exact in ((xi, dyi, True), (xr, dyr, False)):
                dW, db, AW, Ab = S.wgrad_ref(x, None, dy, gt)
                for want_db, ksplit in itertools.product((False, True), splits):
                    xa, xb = (x, None) if ksplit is None else (x[:, :ksplit].contiguous(), x[:, ksplit:].contiguous())
                    c = S.launch_wgrad(xa, dy, x2=xb, gate=gt, want_db=want_db).check()
                    assert (c.db is not None) == want_db
                    if exact:
                        assert torch.equal(c.dW.double(), dW) and (not want_db or torch.equal(c.db.double(), db)), c.what
                        continue
                    bar = (R + 2) * 2.0 ** -24
                    assert bool(((c.dW.double() - dW).abs() <= bar * AW).all()), (c.what, float(((c.dW.double() - dW).abs() / AW).max()))
                    assert not want_db or bool(((c.db.double() - db).abs() <= bar * Ab).all()), c.what
                    again = S.launch_wgrad(xa, dy, x2=xb, gate=gt, want_db=want_db).check()
                    assert torch.equal(again.dW, c.dW) and (not want_db or torch.equal(again.db, c.db)), c.what


@pytest.mark.parametrize("C", (4, 12, 40, 64, 100, 512))
def test_bn_relu_exact_and_guarded(C):
    """(f) sn_bn_relu_forward / _backward at channel counts that are no power of two and row counts whose R C / 4 is no multiple of 256:
    integer z, scales from {1, 2, -1, 0.5, 0}, integer shifts -- the fp32 result is exact, so the mask y > 0 cannot disagree with the
    reference -- bit for bit, with_scale 0 and 1, between guard words.  One real-data case forward: |err| <= 2^-23 (|z scale| + |shift|)."""
    g = S.gen(C)
    scales = torch.tensor([1.0, 2.0, -1.0, 0.5, 0.0], device="cuda")
    for R in (1, 3, 65, 1000):
        z, gr = S.ints(g, -8, 8, R, C), S.ints(g, -8, 8, R, C)
        coef = torch.cat([scales[torch.randint(0, 5, (C,), device="cuda", generator=g)], S.ints(g, -4, 4, C)])
        c = S.launch_bn_relu(z, coef).check()
        assert torch.equal(c.out.double(), S.bn_relu_ref(z, coef)), c.what
        for with_scale in (False, True):
            c = S.launch_bn_relu(z, coef, g=gr, with_scale=with_scale).check()
            assert torch.equal(c.out.double(), S.bn_relu_ref(z, coef, gr, with_scale)), c.what
    z, coef = torch.randn(65, C, device="cuda", generator=g), torch.randn(2 * C, device="cuda", generator=g)
    c = S.launch_bn_relu(z, coef).check()
    mag = (z.double() * coef[:C].double()).abs() + coef[C:].double().abs()
    assert bool(((c.out.double() - S.bn_relu_ref(z, coef)).abs() <= 2.0 ** -23 * mag).all()), c.what
