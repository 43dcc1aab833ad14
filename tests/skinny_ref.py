"""Plain fp64 restatement of the skinny FC entries (sn_skinny_linear, sn_skinny_linear2, sn_skinny_wgrad) and of sn_bn_relu_*, the data
the tests feed them, and a driver that calls the raw entries through samplenet_amd._lib with explicit scratch, counters and output
buffers -- every one a view into a larger buffer filled with a sentinel bit pattern, so that a write outside the view is seen and
cannot fault.  Imported by tests/test_gpu_skinny.py and tools/skinny_floors.py; the references call nothing of the library."""
import torch

# (K, N) -> (S slices, k-steps per wave): the plan of csrc/task_network.hip's skinny_plan, evaluated by hand for these shapes, and
# the branch each of them reaches
PLANS = {
    (1, 1): (1, 1),        # smallest
    (7, 5): (1, 1),        # scalar operand loads, one partial fragment
    (61, 33): (1, 1),      # scalar loads, N crosses a tile
    (64, 7): (1, 1),       # exactly one slice
    (72, 40): (2, 1),      # vector loads with a partial last fragment
    (130, 100): (3, 1),    # scalar loads with S > 1
    (200, 64): (4, 1),
    (576, 33): (9, 1),     # partial second batch of the slice sum
    (584, 70): (5, 2),     # K tail inside a 2-step slice
    (1088, 20): (17, 1),   # three batches
    (1600, 3): (25, 1),    # four batches, one narrow tile
    (1024, 512): (8, 2),
    (2048, 1024): (8, 4),
    (4096, 64): (16, 4),
}
SHAPES = list(PLANS)
ROWS_FULL = (1, 5, 31, 32, 33, 64, 65, 97, 128)
ROWS_FEW = (5, 33, 128)
FULL_ROW_SHAPES = ((61, 33), (576, 33), (584, 70))


def rows_of(shape):
    return ROWS_FULL if shape in FULL_ROW_SHAPES else ROWS_FEW


def row_tiles(R):
    return 1 if R <= 32 else 2 if R <= 64 else 4


# ---- references (fp64, torch only) -----------------------------------------------------------------------------------------------
def linear_ref(x, x2, gate, W, transposed, bias, relu):
    """act(([x | x2] . [gate > 0]) W^T + b) (x W when `transposed`: W is then (K, N)) in fp64, and the component-wise magnitude
    A = |[x | x2] . mask| |W|^T + |b| of the PRE-activation.  -> (out, A)"""
    X = (x if x2 is None else torch.cat([x, x2], dim=1)).double()
    if gate is not None:
        X = X * (gate > 0).double()
    Wt = W.double() if transposed else W.double().t()  # (K, N)
    pre, A = X @ Wt, X.abs() @ Wt.abs()
    if bias is not None:
        pre, A = pre + bias.double(), A + bias.double().abs()
    return (pre.clamp_min(0) if relu else pre), A


def wgrad_ref(x, x2, dy, gate):
    """dW (N, K) = (dy . [gate > 0])^T [x | x2], db (N) = its column sums, and their magnitudes.  -> (dW, db, AW, Ab)"""
    X = (x if x2 is None else torch.cat([x, x2], dim=1)).double()
    dz = dy.double()
    if gate is not None:
        dz = dz * (gate > 0).double()
    return dz.t() @ X, dz.sum(0), dz.abs().t() @ X.abs(), dz.abs().sum(0)


def bn_relu_ref(z, coef, g=None, with_scale=False):
    """y = relu(scale z + shift) per channel (coef = [scale | shift]); with g: dy = g . [y > 0] (times scale when with_scale)."""
    C = z.shape[1]
    sc, sh = coef[:C].double(), coef[C:2 * C].double()
    y = z.double() * sc + sh
    if g is None:
        return y.clamp_min(0)
    dy = g.double() * (y > 0).double()
    return dy * sc if with_scale else dy


def split3_ref(a):
    """The three bf16 planes of fp32 values (round to nearest even, the residual split again), as fp32 tensors."""
    h1 = a.bfloat16().float()
    r1 = a - h1
    h2 = r1.bfloat16().float()
    h3 = (r1 - h2).bfloat16().float()
    return h1, h2, h3


# ---- data ------------------------------------------------------------------------------------------------------------------------
def gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, device="cuda", generator=g).float()


def integer_case(seed, R, K, N):
    """x, W, bias in [-4, 4], gate in [-2, 2] (zeros and negatives present wherever the gate has a few elements): every sum stays
    below 4096 * 16 + 4 < 2^17, so any summation order is exact.  -> x, gate, W (N, K), bias"""
    g = gen(seed)
    x, gate, W, bias = ints(g, -4, 4, R, K), ints(g, -2, 2, R, K), ints(g, -4, 4, N, K), ints(g, -4, 4, N)
    if R * K > 1:  # a zero and a negative gate over non-zero data, whatever the draw
        gate.view(-1)[0], gate.view(-1)[1], x.view(-1)[0], x.view(-1)[1] = 0.0, -2.0, 3.0, -3.0
        W[:, :2] = W[:, :2].abs().clamp_min(1.0)
    return x, gate, W, bias


def real_case(seed, R, K, N):
    """x, W standard normal with W scaled by K^-1/2, the gate a ReLU output with about half zeros.  -> x, gate, W (N, K), bias"""
    g = gen(seed)
    x = torch.randn(R, K, device="cuda", generator=g)
    gate = torch.randn(R, K, device="cuda", generator=g).clamp_min(0)
    W = torch.randn(N, K, device="cuda", generator=g) * K ** -0.5
    return x, gate, W, torch.randn(N, device="cuda", generator=g)


def sparse_rows(g, rows, K, nnz, draw):
    """(rows, K) with at most nnz non-zeros per row at random places, their values from draw(shape)."""
    nnz = min(nnz, K)
    pos = torch.rand(rows, K, device="cuda", generator=g).argsort(dim=1)[:, :nnz]
    return torch.zeros(rows, K, device="cuda").scatter_(1, pos, draw((rows, nnz)))


def k_class(K):
    return 0 if K <= 64 else 1 if K <= 1024 else 2


# ---- guarded buffers -------------------------------------------------------------------------------------------------------------
SENTINEL = 0x7FC5A3E1  # (a NaN when read as fp32: an element the kernel never wrote cannot compare equal to anything)
GUARD = 4096           # words on either side of a view: a multiple of 4 (the views stay 16-byte aligned), wider than any row here


class Guarded:
    """n 32-bit words with GUARD sentinel words before and behind them."""

    def __init__(self, n, dtype=torch.float32, zero=False):
        self.n = n
        self.buf = torch.full((2 * GUARD + n,), SENTINEL, dtype=torch.int32, device="cuda")
        if zero:
            self.buf[GUARD:GUARD + n] = 0
        self.view = self.buf[GUARD:GUARD + n].view(dtype)

    def intact(self):
        return bool((self.buf[:GUARD] == SENTINEL).all()) and bool((self.buf[GUARD + self.n:] == SENTINEL).all())

    def refill(self):
        self.buf[GUARD:GUARD + self.n] = SENTINEL


class Scratch:
    """Slice partials of exactly `nbytes` bytes and `ntiles` zeroed arrival counters, both guarded."""

    def __init__(self, nbytes, ntiles):
        assert nbytes % 4 == 0
        self.part, self.counters = Guarded(nbytes // 4), Guarded(ntiles, torch.int32, zero=True)

    def check(self, what=""):
        assert self.part.intact(), "write outside the scratch: %s" % (what,)
        assert self.counters.intact(), "write outside the counters: %s" % (what,)
        assert not bool(self.counters.view.any()), "counters not left at zero: %s" % (what,)


class Launch:
    """Outputs of one raw call, views into guarded buffers; check() asserts the memory contract after the fact (it synchronises)."""

    def __init__(self, what):
        self.what, self.outs, self.scratch = what, [], None

    def add(self, shape):
        n = 1
        for s in shape:
            n *= s
        gb = Guarded(n)
        self.outs.append(gb)
        return gb.view.view(shape)

    def check(self):
        for gb in self.outs:
            assert gb.intact(), "write outside an output: %s" % (self.what,)
        if self.scratch is not None:
            self.scratch.check(self.what)
        return self


def _lib():
    from samplenet_amd import _lib as L

    return L


def scratch_for(R, K, N):
    return Scratch(_lib().lib.sn_skinny_linear_scratch_bytes(R, K, N), (N + 31) // 32)


def launch_linear(x, W, transposed, x2=None, gate=None, bias=None, relu=False, nsplit=0, want=(True, True), scratch=None):
    """One sn_skinny_linear (no two-part operand) or sn_skinny_linear2 call on the current stream, no synchronisation.
    -> Launch with .out / .out2 (None where not wanted).  scratch: a Scratch to share; None: one of exactly the documented size."""
    L = _lib()
    R, ksplit = x.shape[0], (x.shape[1] if x2 is not None else 0)
    K = x.shape[1] + (x2.shape[1] if x2 is not None else 0)
    N = W.shape[1] if transposed else W.shape[0]
    assert tuple(W.shape) == ((K, N) if transposed else (N, K)) and all(t is None or t.is_contiguous() for t in (x, x2, gate, W, bias))
    call = Launch(("linear", R, K, N, "transposed" if transposed else "plain", "ksplit %d" % ksplit, "gate" if gate is not None else "-",
                   "bias" if bias is not None else "-", "relu" if relu else "-", "nsplit %d" % nsplit, want))
    call.scratch = scratch if scratch is not None else scratch_for(R, K, N)
    if nsplit == 0:
        call.out, call.out2 = call.add((R, N)), None
    else:
        call.out = call.add((R, nsplit)) if want[0] else None
        call.out2 = call.add((R, N - nsplit)) if want[1] else None
    st, p = L.stream_of(x), L.ptr
    part, counters = call.scratch.part.view, call.scratch.counters.view
    if x2 is None and nsplit == 0:
        rc = L.lib.sn_skinny_linear(R, K, N, p(x), p(gate), p(W), int(transposed), p(bias), int(relu), p(call.out), p(part), p(counters), st)
    else:
        rc = L.lib.sn_skinny_linear2(R, K, N, p(x), p(x2), ksplit, p(gate), p(W), int(transposed), p(bias), int(relu), p(call.out),
                                     p(call.out2), nsplit, p(part), p(counters), st)
    L.check(rc, str(call.what))
    return call


def launch_wgrad(x, dy, x2=None, gate=None, want_db=True):
    L = _lib()
    R, N = dy.shape
    ksplit = x.shape[1] if x2 is not None else 0
    K = x.shape[1] + (x2.shape[1] if x2 is not None else 0)
    call = Launch(("wgrad", R, K, N, "ksplit %d" % ksplit, "gate" if gate is not None else "-", "db" if want_db else "-"))
    call.dW = call.add((N, K))
    call.db = call.add((N,)) if want_db else None
    p = L.ptr
    L.check(L.lib.sn_skinny_wgrad(R, K, N, p(x), p(x2), ksplit, p(dy), p(gate), p(call.dW), p(call.db), L.stream_of(x)), str(call.what))
    return call


def launch_bn_relu(z, coef, g=None, with_scale=False):
    """z, coef (and g) must themselves be 16-byte aligned (fresh tensors are)."""
    L = _lib()
    R, C = z.shape
    call = Launch(("bn_relu", R, C, "backward" if g is not None else "forward", "scale" if with_scale else "-"))
    call.out = call.add((R, C))
    p, st = L.ptr, L.stream_of(z)
    if g is None:
        rc = L.lib.sn_bn_relu_forward(R, C, p(z), p(coef), p(call.out), st)
    else:
        rc = L.lib.sn_bn_relu_backward(R, C, p(z), p(coef), p(g), int(with_scale), p(call.out), st)
    L.check(rc, str(call.what))
    return call
