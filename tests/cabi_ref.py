"""Test helper for the C-ABI contract tests (tests/test_gpu_cabi_contract.py, tests/test_cabi_arguments.py): plain fp64
restatements of the geometric operations of include/samplenet_hip.h (softmax weights, weighted gather, index-add, the soft
projection and its gradients, the simplification / Chamfer-mean losses, the PCRNet head, quaternion rotation), the input
recipes the existing GPU tests use, the poison-and-guard buffers that prove "overwritten" / "may be NULL" sentences, and the small
helpers every direct test of an entry point needs (stream, bits, invert).
Lives in tests/ on purpose: nothing here is a product route."""
import numpy as np
import torch

POISON = 0x7FFFFFFF  # a quiet NaN as float32, INT_MAX as int32: no kernel in scope produces either
GUARD = 64           # guard words on either side of every output buffer (keeps the payload 256-byte aligned)

BAD_ARGUMENT, UNSUPPORTED = 10001, 10002
BNC, BCN = 0, 1


# ------------------------------------------------------------------------------------------------ inputs
def clouds(seed, b, n, m, dup=True):
    """The recipe of tests/test_gpu_geometry.py: uniform clouds with exact duplicates and one zero distance."""
    rng = np.random.default_rng(seed)
    x1 = rng.random((b, n, 3), dtype=np.float32) - 0.5
    x2 = rng.random((b, m, 3), dtype=np.float32) - 0.5
    if dup and n > 12 and m > 12:
        x2[:, 3] = x2[:, 9]
        x2[:, 11] = x2[:, 9]
        x1[:, 2] = x1[:, 7]
        x1[0, 5] = x2[0, 4]
    return x1, x2


def tie_clouds(seed, b, n, m):
    """clouds() plus, when n > 300, the 40 coincident points of test_knn_matches_oracle (ties on the K-th boundary)."""
    P, Q = clouds(seed, b, n, m)
    if n > 300:
        P[:, 100:140] = P[:, 100:101]
        Q[:, 0] = P[:, 100]
    return P, Q


def surface_queries(seed, b, n, m, cluster=False):
    """test_soft_project_fused_vs_oracle's recipe: queries = cloud points + 0.02 sigma noise.  cluster: 24 coincident points and
    a third of the queries next to them, so that many queries name the same destination points."""
    P, _ = clouds(seed, b, n, m)
    rng = np.random.default_rng(seed + 1)
    src = P[:, np.arange(m) % n]
    if cluster and n > 40:
        P[:, 8:32] = P[:, 8:9]
        src = src.copy()
        src[:, ::3] = P[:, 8:9]
    Q = (src + 0.02 * rng.standard_normal((b, m, 3))).astype(np.float32)
    return P, Q


def sigma_of(T, min_sigma):
    """sigma = max(T*T, min_sigma) as the kernels form it: in float32."""
    return float(max(np.float32(T) * np.float32(T), np.float32(min_sigma)))


def t(x, layout=BNC):
    """(b, n, 3) numpy -> contiguous numpy in the selected layout."""
    return np.ascontiguousarray(x if layout == BNC else x.transpose(0, 2, 1))


def back(x, layout):
    """array or tensor in `layout` -> (b, n, 3)."""
    if layout == BNC:
        return x
    return x.transpose(1, 2) if isinstance(x, torch.Tensor) else x.transpose(0, 2, 1)


# ------------------------------------------------------------------------------------------------ guarded buffers
class Guarded:
    """A device buffer pre-filled with POISON, with GUARD poisoned words in front and behind."""

    def __init__(self, shape, dtype=torch.float32, fill=None, device="cuda"):
        self.shape = tuple(int(s) for s in shape)
        self.n = int(np.prod(self.shape)) if self.shape else 1
        self.raw = torch.full((self.n + 2 * GUARD,), POISON, dtype=torch.int32, device=device)
        self.dtype = dtype
        if fill is not None:
            self.view().copy_(torch.as_tensor(fill).to(device=device, dtype=dtype).reshape(self.shape))

    def view(self):
        inner = self.raw[GUARD:GUARD + self.n]
        return (inner if self.dtype == torch.int32 else inner.view(self.dtype)).view(self.shape)

    def ptr(self):
        return self.raw.data_ptr() + 4 * GUARD

    def words(self):
        return self.raw[GUARD:GUARD + self.n]

    def guards_intact(self):
        return bool((self.raw[:GUARD] == POISON).all()) and bool((self.raw[GUARD + self.n:] == POISON).all())

    def fully_written(self):
        return not bool((self.words() == POISON).any())

    def untouched(self):
        return bool((self.raw == POISON).all())

    def check(self, what=""):
        assert self.guards_intact(), "%s: a guard word changed" % what
        assert self.fully_written(), "%s: %d of %d elements were not written" % (what, int((self.words() == POISON).sum()), self.n)
        return self.view()

    def numpy(self):
        return self.view().cpu().numpy()


def arg(x):
    """ctypes argument of a tensor / Guarded buffer / None / plain number."""
    if x is None:
        return None
    if isinstance(x, Guarded):
        return x.ptr()
    if isinstance(x, torch.Tensor):
        return x.data_ptr()
    return x


def stream():
    """The current stream, as the entry points take it."""
    return torch.cuda.current_stream().cuda_stream


def bits(a):
    """float32 values as their int32 bit patterns: array_equal on these tells -0 from +0 and one NaN from another."""
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def invert(lib, b, n, ne, idx):
    """sn_gather_invert of a device idx (b,ne) int32 into plain device buffers -> start (b,n+1), order (b,ne)."""
    start, order = torch.empty(b, n + 1, device="cuda", dtype=torch.int32), torch.empty(b, ne, device="cuda", dtype=torch.int32)
    assert lib.sn_gather_invert(b, n, ne, idx.data_ptr(), start.data_ptr(), order.data_ptr(), stream()) == 0
    return start, order


# ------------------------------------------------------------------------------------------------ fp64 references
def _gather(P, idx):
    """P (b,n,c) , idx (b,m,k) -> (b,m,k,c)."""
    b = P.shape[0]
    return P[torch.arange(b).view(b, 1, 1), idx.long()]


def soft_weights(P, Q, idx, sigma):
    """fp64 softmax_k(-|P[idx] - Q|^2 / sigma): P (b,n,3), Q (b,m,3), idx (b,m,k) numpy -> (b,m,k) float64."""
    P, Q = torch.from_numpy(np.asarray(P)).double(), torch.from_numpy(np.asarray(Q)).double()
    nb = _gather(P, torch.from_numpy(np.asarray(idx)))
    d = ((nb - Q[:, :, None, :]) ** 2).sum(-1)
    return torch.softmax(-d / sigma, dim=-1).numpy()


def weighted_gather(X, idx, w):
    """fp64 out[b,c,j] = sum_k w[b,j,k] X[b,c,idx[b,j,k]]: X (b,c,n), idx / w (b,m,k) -> (b,c,m)."""
    X = torch.from_numpy(np.asarray(X)).double().transpose(1, 2)  # (b,n,c)
    nb = _gather(X, torch.from_numpy(np.asarray(idx)))            # (b,m,k,c)
    out = (nb * torch.from_numpy(np.asarray(w)).double()[..., None]).sum(2)
    return out.transpose(1, 2).contiguous().numpy()


def index_add(n, idx, src):
    """fp64 dst[b, idx[b,e], :] += src[b,e,:]: idx (b,ne), src (b,ne,c) -> (dst (b,n,c), hits (b,n), sum of |terms| (b,n,c))."""
    idx, src = np.asarray(idx).astype(np.int64), np.asarray(src, dtype=np.float64)
    b, ne, c = src.shape
    dst, sab, hits = np.zeros((b, n, c)), np.zeros((b, n, c)), np.zeros((b, n))
    for i in range(b):
        np.add.at(dst[i], idx[i], src[i])
        np.add.at(sab[i], idx[i], np.abs(src[i]))
        np.add.at(hits[i], idx[i], 1.0)
    return dst, hits, sab


def soft_project(P, Q, idx, sigma, grad_proj=None):
    """fp64 soft projection of soft_projection.py:138-152 on (b,n,3) / (b,m,3) clouds and, with grad_proj (b,m,3), its gradients
    by autograd: -> proj (b,m,3), w (b,m,k) [, grad_P (b,n,3), grad_Q (b,m,3), grad_sigma]."""
    P = torch.from_numpy(np.asarray(P)).double().requires_grad_(True)
    Q = torch.from_numpy(np.asarray(Q)).double().requires_grad_(True)
    sg = torch.tensor(float(sigma), dtype=torch.float64, requires_grad=True)
    nb = _gather(P, torch.from_numpy(np.asarray(idx)))
    d = ((nb - Q[:, :, None, :]) ** 2).sum(-1)
    w = torch.softmax(-d / sg, dim=-1)
    proj = (w[..., None] * nb).sum(2)
    if grad_proj is None:
        return proj.detach().numpy(), w.detach().numpy()
    gP, gQ, gs = torch.autograd.grad(proj, [P, Q, sg], torch.from_numpy(np.asarray(grad_proj)).double())
    return proj.detach().numpy(), w.detach().numpy(), gP.numpy(), gQ.numpy(), float(gs)


def soft_weights_backward(P, Q, idx, sigma, grad_w):
    """fp64 gradients of soft_weights() for an upstream grad_w (b,m,k): -> grad_P (b,n,3), grad_Q (b,m,3), grad_sigma."""
    P = torch.from_numpy(np.asarray(P)).double().requires_grad_(True)
    Q = torch.from_numpy(np.asarray(Q)).double().requires_grad_(True)
    sg = torch.tensor(float(sigma), dtype=torch.float64, requires_grad=True)
    nb = _gather(P, torch.from_numpy(np.asarray(idx)))
    d = ((nb - Q[:, :, None, :]) ** 2).sum(-1)
    w = torch.softmax(-d / sg, dim=-1)
    gP, gQ, gs = torch.autograd.grad(w, [P, Q, sg], torch.from_numpy(np.asarray(grad_w)).double())
    return gP.numpy(), gQ.numpy(), float(gs)


def weighted_gather_backward(X, idx, w, grad_out):
    """fp64: X (b,c,n), idx / w (b,m,k), grad_out (b,c,m) -> grad_w (b,m,k), grad_X (b,c,n)."""
    X = torch.from_numpy(np.asarray(X)).double().requires_grad_(True)
    w = torch.from_numpy(np.asarray(w)).double().requires_grad_(True)
    nb = _gather(X.transpose(1, 2), torch.from_numpy(np.asarray(idx)))
    out = (nb * w[..., None]).sum(2).transpose(1, 2)
    gw, gX = torch.autograd.grad(out, [w, X], torch.from_numpy(np.asarray(grad_out)).double())
    return gw.numpy(), gX.numpy()


def simplification_loss(x1, x2, i1, i2, weight, with_max=True, grad_loss=1.0):
    """fp64 loss = mean(d1) + [mean_b max_m d1] + weight * mean(d2) with d1 = |x1 - x2[i1]|^2, d2 = |x2 - x1[i2]|^2
    (samplenet.py:171-181; with_max=False: main.py:573-577) -> loss, grad_x1, grad_x2 (scaled by grad_loss)."""
    a = torch.from_numpy(np.asarray(x1)).double().requires_grad_(True)
    c = torch.from_numpy(np.asarray(x2)).double().requires_grad_(True)
    b = a.shape[0]
    ar = torch.arange(b).view(b, 1)
    d1 = ((a - c[ar, torch.from_numpy(np.asarray(i1)).long()]) ** 2).sum(-1)
    d2 = ((c - a[ar, torch.from_numpy(np.asarray(i2)).long()]) ** 2).sum(-1)
    loss = d1.mean() + weight * d2.mean()
    if with_max:
        loss = loss + d1.max(dim=1).values.mean()
    ga, gc = torch.autograd.grad(loss * grad_loss, [a, c])
    return float(loss.detach()), ga.numpy(), gc.numpy()


def pcrnet_head(y, g_twist=None, g_quat=None, g_qnorm=None):
    """fp64 twist (B,7) = [normalize(y[:, :4]) | y[:, 4:]], quat, qnorm = mean_b (|y[:, :4]|^2 - 1)^2 and g_y."""
    y = torch.from_numpy(np.asarray(y)).double().requires_grad_(True)
    q = y[:, :4] / y[:, :4].norm(dim=1, keepdim=True).clamp_min(1e-12)
    twist = torch.cat([q, y[:, 4:]], 1)
    qnorm = ((y[:, :4] ** 2).sum(1) - 1.0).pow(2).mean()
    tot = 0.0 * y.sum()
    if g_twist is not None:
        tot = tot + (twist * torch.from_numpy(np.asarray(g_twist)).double()).sum()
    if g_quat is not None:
        tot = tot + (q * torch.from_numpy(np.asarray(g_quat)).double()).sum()
    if g_qnorm is not None:
        tot = tot + qnorm * float(g_qnorm)
    (gy,) = torch.autograd.grad(tot, [y])
    return twist.detach().numpy(), q.detach().numpy(), float(qnorm.detach()), gy.numpy()


def qrot(quat, v, grad_out=None):
    """fp64 quaternion.py:35-53: out = v + 2 (w (qv x v) + qv x (qv x v)), quat (B,4) in (w,x,y,z), v (B,N,3); gradients."""
    q = torch.from_numpy(np.asarray(quat)).double().requires_grad_(True)
    x = torch.from_numpy(np.asarray(v)).double().requires_grad_(True)
    qv = q[:, None, 1:].expand_as(x)
    uv = torch.cross(qv, x, dim=2)
    uuv = torch.cross(qv, uv, dim=2)
    out = x + 2 * (q[:, None, :1] * uv + uuv)
    if grad_out is None:
        return out.detach().numpy()
    gq, gv = torch.autograd.grad(out, [q, x], torch.from_numpy(np.asarray(grad_out)).double())
    return out.detach().numpy(), gq.numpy(), gv.numpy()
