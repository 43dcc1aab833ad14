"""The fp64 reference of one Adam step and the single-step rounding bound samplenet_amd.optim.Adam (csrc/optimizer.hip) is held to;
imported by tests/test_gpu_adam.py and tests/test_gpu_adam_engine.py.  The reference is torch.optim.Adam(foreach=False) on float64 CPU
copies of the device's fp32 state; for tf_epsilon=True it is tf.train.AdamOptimizer's documented update restated in fp64 (TensorFlow
itself cannot run here).

The bound, element by element, no exemptions, u = 2^-24, from the operation order pinned in csrc/optimizer.hip:
    g1 = fl(g gs + wd p)            formed in fp64, rounded once: g1 (1 + d), |d| <= u (+ 2^-52), relative to g1 ITSELF
    m' = fma(fl(b1), m, fl(fl(1 - b1) g1))
         (1 - b1) g1 carries three factors (g1, the coefficient's representation, the product), b1 m one (representation), the fma
         rounds m' once:  |m'_hip - m'| <= u (3 (1 - b1)|g1| + b1 |m| + |m'|) <= 4 u A,   A = b1 |m| + (1 - b1)(gs |g| + wd |p|)
    v' = fma(fl(b2), v, fl(fl(fl(1 - b2) g1) g1))
         the second term carries five factors (g1 twice, representation, two products), the first one, the fma one; all terms are
         non-negative:  |v'_hip - v'| <= u (5 (1 - b2) g1^2 + b2 v + v') <= 6 u v'
    den = fl(fl(sqrt(v')) / fl(sqrt(bc2))) + fl(eps)   [torch form]
         sqrt halves v's 6 u and rounds (4 u), the divisor's representation and the division (6 u), eps' representation and the sum:
         |den_hip - D| <= 7 u D,   D = sqrt(v' / bc2) + eps        (TensorFlow form: no division, 5 u)
    p' = fma(-fl(step), fl(m' / den), p)
         the quotient: 4 u A / D from m', 7 u |m'| / D <= 7 u A / D from den, its own rounding u: 12 u A / D; step's representation
         one more; the fma rounds p' once:  |p'_hip - p'| <= u |p'| + 13 u A step / D,  step = lr / bc1  (TF: lr sqrt(bc2) / bc1)
    so the constants are 4, 6 and 13 (the issue's sketch counts 12 for the last: it does not count the representation of lr / bc1).
    Products of at most 13 factors (1 + d): the neglected higher-order terms are below 13^2 u^2 < 32 u times the first-order bound --
    the factor (1 + 32 u) below.  bc1, bc2 come from fp64 running products (relative error t 2^-53: nothing against u).
"""
import torch

U = 2.0 ** -24
CM, CV, CP = 4.0, 6.0, 13.0
SLACK = 1.0 + 32.0 * U
LR, BETAS, EPS = 1e-3, (0.9, 0.999), 1e-8


def reference_step(p, g, m, v, t, lr=LR, betas=BETAS, eps=EPS, wd=0.0, tf=False, gs=1.0):
    """One update in fp64 on the CPU from fp32 state (lists of tensors; g[i] None: no gradient) -> p', m', v' lists in fp64 and the
    bound's ingredients A and step / D per tensor."""
    b1, b2 = betas
    p64 = [torch.nn.Parameter(x.double().cpu()) for x in p]
    g64 = [None if x is None else x.double().cpu() * gs for x in g]
    m64, v64 = [x.double().cpu() for x in m], [x.double().cpu() for x in v]
    bc1, bc2 = 1.0 - b1 ** (t + 1), 1.0 - b2 ** (t + 1)
    A = [None if gi is None else b1 * mi.abs() + (1 - b1) * (gi.abs() + wd * pi.detach().abs()) for pi, gi, mi in zip(p64, g64, m64)]
    if not tf:
        ref = torch.optim.Adam(p64, lr=lr, betas=betas, eps=eps, weight_decay=wd, foreach=False)
        for pi, gi, mi, vi in zip(p64, g64, m64, v64):
            pi.grad = gi
            ref.state[pi] = {"step": torch.tensor(float(t)), "exp_avg": mi, "exp_avg_sq": vi}  # (updated in place)
        ref.step()
        for pi in p64:
            if pi.grad is not None:
                assert int(ref.state[pi]["step"]) == t + 1
        scale = [None if gi is None else (lr / bc1) / ((vi / bc2).sqrt() + eps) for gi, vi in zip(g64, v64)]
    else:  # tf.train.AdamOptimizer: lr_t = lr sqrt(1 - b2^t) / (1 - b1^t); variable -= lr_t m_t / (sqrt(v_t) + epsilon)
        scale = []
        for i, (pi, gi) in enumerate(zip(p64, g64)):
            if gi is None:
                scale.append(None)
                continue
            g1 = gi + wd * pi.detach()
            m64[i] = b1 * m64[i] + (1 - b1) * g1
            v64[i] = b2 * v64[i] + (1 - b2) * g1 * g1
            lr_t = lr * bc2 ** 0.5 / bc1
            pi.data = pi.detach() - lr_t * m64[i] / (v64[i].sqrt() + eps)
            scale.append(lr_t / (v64[i].sqrt() + eps))
    return [x.detach() for x in p64], m64, v64, A, scale


def check_step(before, after, grads, what="", **kw):
    """after (device state) against one reference step from before, within the bound; untouched where the gradient is None."""
    p0, m0, v0, t0 = before
    p1, m1, v1, t1 = after
    assert t1 == t0 + 1, what
    pr, mr, vr, A, scale = reference_step(p0, grads, m0, v0, t0, **kw)
    worst = [0.0, 0.0, 0.0]
    for i in range(len(p0)):
        if grads[i] is None:
            assert torch.equal(p1[i], p0[i]) and torch.equal(m1[i], m0[i]) and torch.equal(v1[i], v0[i]), (what, i)
            continue
        ph, mh, vh = p1[i].double().cpu(), m1[i].double().cpu(), v1[i].double().cpu()
        assert torch.isfinite(ph).all() and torch.isfinite(mh).all() and torch.isfinite(vh).all(), (what, i)
        em, bm = (mh - mr[i]).abs(), CM * U * A[i] * SLACK
        ev, bv = (vh - vr[i]).abs(), CV * U * vr[i] * SLACK
        ep, bp = (ph - pr[i]).abs(), (U * pr[i].abs() + CP * U * A[i] * scale[i]) * SLACK
        for k, (e, b) in enumerate(((em, bm), (ev, bv), (ep, bp))):
            ratio = float((e / b.clamp_min(1e-300)).max())
            worst[k] = max(worst[k], ratio)
        assert bool((em <= bm).all()), (what, "m", i, float((em / bm.clamp_min(1e-300)).max()))
        assert bool((ev <= bv).all()), (what, "v", i, float((ev / bv.clamp_min(1e-300)).max()))
        assert bool((ep <= bp).all()), (what, "p", i, float((ep / bp.clamp_min(1e-300)).max()))
    print("adam %s: worst error / bound  m %.3f  v %.3f  p %.3f" % (what, *worst))
    return pr, mr, vr
