"""The fp64 references of one SGD / RMSprop step and the single-step rounding bounds samplenet_amd.optim.SGD and RMSprop
(csrc/optimizer.hip: sn_sgd_update, sn_rmsprop_update) are held to; imported by tests/test_gpu_optim.py and
tests/test_gpu_optim_engine.py.  The references are torch.optim.SGD(foreach=False) and torch.optim.RMSprop(foreach=False) on float64 CPU
copies of the device's fp32 state, ALWAYS ONE STEP FROM IDENTICAL STATE (as tests/adam_ref.py).

The bounds, element by element, no exemptions, no measured tolerance, u = 2^-24, from the operation order pinned in csrc/optimizer.hip.
"Representation" is the one rounding of a host fp64 coefficient to fp32: fl(lr), fl(mu), fl(1 - dampening), fl(alpha), fl(1 - alpha),
fl(eps) each carry one factor (1 + d), |d| <= u.  G = gs |g| + wd |p| >= |g1|.
    g1 = fl(g gs + wd p)            formed in fp64, rounded once: g1 (1 + d), |d| <= u (+ 2^-52)

  SGD
    b' = fma(fl(mu), b, fl(fl(1 - dampening) g1))                                                  [momentum != 0, t > 0]
         (1 - dampening) g1 carries three factors (g1, the coefficient's representation, the product), mu b one (representation), the
         fma rounds b' once:  |b'_hip - b'| <= u (3 (1 - dampening)|g1| + mu |b| + |b'|) <= 4 u Ab,   Ab = mu |b| + (1 - dampening) G
    b' = g1                         [t == 0: torch clones the gradient, the buffer's content and dampening are ignored]
         one factor: u |g1| <= u Ab with Ab = G -- held to the same constant 4.
    d  = b'                         |d_hip - d| <= 4 u Ab,  |d| <= Ab                               [no Nesterov]
    d  = fma(fl(mu), b', g1)        mu's representation u mu |b'|, b's error 4 u mu Ab, g1's u |g1|, the fma u |d|, with |b'| <= Ab
         and |d| <= Ad = mu Ab + G:  |d_hip - d| <= u (2 mu Ab + 2 G + 4 mu Ab) <= 6 u Ad           [Nesterov]
    d  = g1                         |d_hip - d| <= u G,  |d| <= G                                   [momentum == 0]
    p' = fma(-fl(lr), d, p)         lr's representation u lr |d|, d's error, the fma rounds p' once:
         |p'_hip - p'| <= u |p'| + C u lr A   with (C, A) = (5, Ab), (7, Ad), (2, G) in the three cases.

  RMSprop
    s' = fma(fl(alpha), s, fl(fl(fl(1 - alpha) g1) g1))
         the second term carries five factors (g1 twice, representation, two products), the first one, the fma one; all terms are
         non-negative:  |s'_hip - s'| <= u (5 (1 - alpha) g1^2 + alpha s + s') <= 6 u s'
    den = fl(sqrt(s')) + fl(eps)    sqrt halves s's 6 u and rounds (4 u on the root), eps' representation, the sum:
         |den_hip - D| <= 5 u D,   D = sqrt(s') + eps
    q  = fl(g1 / den)               g1's u, den's 5 u, the division:  |q_hip - q| <= 7 u Q,   Q = G / D >= |q|
    p' = fma(-fl(lr), q, p)         lr's representation one more:  |p'_hip - p'| <= u |p'| + 8 u lr Q               [momentum == 0]
    b' = fma(fl(mu), b, q)          mu's representation u mu |b|, q's 7 u Q, the fma u |b'| <= u (mu |b| + Q):
         |b'_hip - b'| <= u (2 mu |b| + 8 Q) <= 8 u Ab,   Ab = mu |b| + Q >= |b'|                                   [momentum != 0]
    p' = fma(-fl(lr), b', p)        |p'_hip - p'| <= u |p'| + 9 u lr Ab

Products of at most 9 factors (1 + d): the neglected higher-order terms are below 9^2 u^2 < 32 u times the first-order bound -- the
factor (1 + 32 u) below, which also covers the fp64 reference's own roundings (2^-53 per operation, 2^-29 u).
"""
import torch

U = 2.0 ** -24
SLACK = 1.0 + 32.0 * U
SGD_CB, SGD_CP_PLAIN, SGD_CP_NESTEROV, SGD_CP_NOMOM = 4.0, 5.0, 7.0, 2.0
RMS_CS, RMS_CP_NOMOM, RMS_CB, RMS_CP_MOM = 6.0, 8.0, 8.0, 9.0


def _f64(xs):
    return [None if x is None else x.detach().double().cpu() for x in xs]


def reference_sgd_step(p, g, b, t, lr=1e-3, momentum=0.0, dampening=0.0, wd=0.0, nesterov=False, gs=1.0):
    """One torch.optim.SGD(foreach=False) step in fp64 on the CPU from fp32 state (lists of tensors; g[i] None: no gradient; b None
    or b[i] None or t == 0: the parameter has no momentum buffer yet) -> p', b' lists (b'[i] None where torch holds none) and the
    bound's ingredients per tensor: Ab, and (C, A) of the parameter bound."""
    n = len(p)
    p64 = [torch.nn.Parameter(x) for x in _f64(p)]
    g64 = [None if x is None else x * gs for x in _f64(g)]
    b64 = _f64(b) if (b is not None and t > 0) else [None] * n
    G = [None if gi is None else gi.abs() + wd * pi.detach().abs() for pi, gi in zip(p64, g64)]
    Ab, CA = [], []
    for i in range(n):
        if g64[i] is None:
            Ab.append(None), CA.append(None)
        elif momentum == 0:
            Ab.append(None), CA.append((SGD_CP_NOMOM, G[i]))
        else:
            ab = G[i] if b64[i] is None else momentum * b64[i].abs() + (1.0 - dampening) * G[i]
            Ab.append(ab)
            CA.append((SGD_CP_NESTEROV, momentum * ab + G[i]) if nesterov else (SGD_CP_PLAIN, ab))
    ref = torch.optim.SGD(p64, lr=lr, momentum=momentum, dampening=dampening, weight_decay=wd, nesterov=nesterov, foreach=False)
    for pi, gi, bi in zip(p64, g64, b64):
        pi.grad = gi
        if bi is not None:
            ref.state[pi]["momentum_buffer"] = bi.clone()
    ref.step()
    bout = [ref.state[pi].get("momentum_buffer") if pi in ref.state else None for pi in p64]
    return [x.detach() for x in p64], bout, Ab, CA


def check_sgd_step(before, after, grads, what="", **kw):
    """after (device state) against one reference step from before, within the bound; untouched where the gradient is None.
    before / after: (p list, b list or None, t).  before's b[i] may be None: a parameter that has no buffer yet."""
    p0, b0, t0 = before
    p1, b1, t1 = after
    assert t1 == t0 + 1, what
    lr = kw.get("lr", 1e-3)
    pr, br, Ab, CA = reference_sgd_step(p0, grads, b0, t0, **kw)
    worst = [0.0, 0.0]
    for i in range(len(p0)):
        if grads[i] is None:
            assert torch.equal(p1[i], p0[i]), (what, i)
            assert b1 is None or b0 is None or b0[i] is None or torch.equal(b1[i], b0[i]), (what, i)
            continue
        ph = p1[i].double().cpu()
        assert torch.isfinite(ph).all(), (what, i)
        if kw.get("momentum", 0.0) != 0:
            bh = b1[i].double().cpu()
            assert torch.isfinite(bh).all(), (what, i)
            eb, bb = (bh - br[i]).abs(), SGD_CB * U * Ab[i] * SLACK
            worst[0] = max(worst[0], float((eb / bb.clamp_min(1e-300)).max()))
            assert bool((eb <= bb).all()), (what, "b", i, float((eb / bb.clamp_min(1e-300)).max()))
        else:
            assert b1 is None, what
        c, a = CA[i]
        ep, bp = (ph - pr[i]).abs(), (U * pr[i].abs() + c * U * lr * a) * SLACK
        worst[1] = max(worst[1], float((ep / bp.clamp_min(1e-300)).max()))
        assert bool((ep <= bp).all()), (what, "p", i, float((ep / bp.clamp_min(1e-300)).max()))
    print("sgd %s: worst error / bound  b %.3f  p %.3f" % (what, *worst))
    return pr, br


def reference_rmsprop_step(p, g, s, b, t, lr=1e-2, alpha=0.99, eps=1e-8, wd=0.0, momentum=0.0, gs=1.0):
    """One torch.optim.RMSprop(foreach=False) step in fp64 on the CPU from fp32 state -> p', s', b' lists (b' None without momentum)
    and the bound's ingredients per tensor: Q = G / D and Ab = mu |b| + Q (None without momentum)."""
    p64 = [torch.nn.Parameter(x) for x in _f64(p)]
    g64 = [None if x is None else x * gs for x in _f64(g)]
    s64 = [x.clone() for x in _f64(s)]
    b64 = [x.clone() for x in _f64(b)] if momentum > 0 else None
    G = [None if gi is None else gi.abs() + wd * pi.detach().abs() for pi, gi in zip(p64, g64)]
    babs = None if b64 is None else [x.abs() for x in b64]
    ref = torch.optim.RMSprop(p64, lr=lr, alpha=alpha, eps=eps, weight_decay=wd, momentum=momentum, foreach=False)
    for i, (pi, gi) in enumerate(zip(p64, g64)):
        pi.grad = gi
        st = {"step": torch.tensor(float(t)), "square_avg": s64[i]}  # (updated in place)
        if momentum > 0:
            st["momentum_buffer"] = b64[i]
        ref.state[pi] = st
    ref.step()
    Q, Ab = [], []
    for i, gi in enumerate(g64):
        if gi is None:
            Q.append(None), Ab.append(None)
            continue
        assert int(ref.state[p64[i]]["step"]) == t + 1
        Q.append(G[i] / (s64[i].sqrt() + eps))
        Ab.append(momentum * babs[i] + Q[-1] if momentum > 0 else None)
    return [x.detach() for x in p64], s64, b64, Q, Ab


def check_rmsprop_step(before, after, grads, what="", **kw):
    """before / after: (p list, s list, b list or None, t)."""
    p0, s0, b0, t0 = before
    p1, s1, b1, t1 = after
    assert t1 == t0 + 1, what
    lr, mom = kw.get("lr", 1e-2), kw.get("momentum", 0.0)
    pr, sr, br, Q, Ab = reference_rmsprop_step(p0, grads, s0, b0, t0, **kw)
    worst = [0.0, 0.0, 0.0]
    for i in range(len(p0)):
        if grads[i] is None:
            assert torch.equal(p1[i], p0[i]) and torch.equal(s1[i], s0[i]) and (mom == 0 or torch.equal(b1[i], b0[i])), (what, i)
            continue
        ph, sh = p1[i].double().cpu(), s1[i].double().cpu()
        assert torch.isfinite(ph).all() and torch.isfinite(sh).all(), (what, i)
        checks = [("s", (sh - sr[i]).abs(), RMS_CS * U * sr[i] * SLACK)]
        if mom > 0:
            bh = b1[i].double().cpu()
            assert torch.isfinite(bh).all(), (what, i)
            checks.append(("b", (bh - br[i]).abs(), RMS_CB * U * Ab[i] * SLACK))
            checks.append(("p", (ph - pr[i]).abs(), (U * pr[i].abs() + RMS_CP_MOM * U * lr * Ab[i]) * SLACK))
        else:
            assert b1 is None, what
            checks.append(("p", (ph - pr[i]).abs(), (U * pr[i].abs() + RMS_CP_NOMOM * U * lr * Q[i]) * SLACK))
        for name, e, bnd in checks:
            ratio = float((e / bnd.clamp_min(1e-300)).max())
            k = "sbp".index(name)
            worst[k] = max(worst[k], ratio)
            assert bool((e <= bnd).all()), (what, name, i, ratio)
    print("rmsprop %s: worst error / bound  s %.3f  b %.3f  p %.3f" % (what, *worst))
    return pr, sr, br
