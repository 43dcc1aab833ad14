"""What the SGD and RMSprop updates cost, alone and as the last node of the sampler's captured training step, beside Adam's -- on the
sampler's real parameter set (the headline configuration of bench.py: B = 32, N = 1024, M = 64, K = 8; ~30 tensors, 249,793 floats).

    python tools/optim_bench.py > profiles/optim/optim_bench.txt

Part 1 -- each update alone, gradients resident in the reducer's bucket: samplenet_amd.optim.SGD (momentum 0.9) against
torch.optim.SGD in its default, foreach=True and fused=True forms, and samplenet_amd.optim.RMSprop against torch.optim.RMSprop in its
default and foreach=True forms (it has no fused form).  Per form:
    enqueue   host time per step() with the device left to drain on its own (a host clock around the calls, no synchronise inside)
    complete  host clock around the same number of calls ENDING in a synchronise: what a training loop pays per step -- the larger of
              the host's launch path and the device's work
Part 2 -- the captured training step (engine.SamplerTrainStep on an 8-entry input ring, as bench.py runs it) with no optimizer, and with
Adam, SGD (momentum 0.9) and RMSprop as the last node of its graph.  The legs are alternated round by round; every figure is
milliseconds per step to completion.  The summary gives each update's increment over the no-optimizer leg OF THE SAME ROUND (mean and
range over the rounds), and the spread between the repeated legs of one variant, which is what a difference between two increments has
to exceed before it means anything.  SGD moves 5 arrays per element (read p, g, b; write p, b) and RMSprop 5 (7 with momentum), Adam 7.
"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, N, M, K = 32, 1024, 64, 8
FORMS = ("hip-sgd", "torch-sgd-default", "torch-sgd-foreach", "torch-sgd-fused", "hip-rmsprop", "torch-rmsprop-default",
         "torch-rmsprop-foreach")
LEGS = ("no-update", "adam", "sgd", "rmsprop")


def make_net():
    from samplenet_amd import SampleNet

    torch.manual_seed(0)
    return SampleNet(M, 128, group_size=K, initial_temperature=1.0, is_temperature_trainable=True, min_sigma=1e-2,
                     input_shape="bnc", output_shape="bnc").cuda().train()


def make_opt(form, params):
    from samplenet_amd import optim

    if form == "hip-sgd":
        return optim.SGD(params, lr=1e-3, momentum=0.9)
    if form == "hip-rmsprop":
        return optim.RMSprop(params, lr=1e-3)
    kw = {"default": {}, "foreach": {"foreach": True}, "fused": {"fused": True}}[form.split("-")[2]]
    if form.startswith("torch-sgd"):
        return torch.optim.SGD(params, lr=1e-3, momentum=0.9, **kw)
    return torch.optim.RMSprop(params, lr=1e-3, **kw)


def timed(fn, n):
    """-> (enqueue ms, complete ms) per call over n calls."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        fn(i)
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return (t1 - t0) / n * 1e3, (t2 - t0) / n * 1e3


def part1(steps, rounds):
    from samplenet_amd.parallel import FlatGradAllReducer

    print("part 1: each update alone (%d steps per round, %d alternated rounds)" % (steps, rounds))
    setups = {}
    for form in FORMS:
        net = make_net()
        red = FlatGradAllReducer(net)
        red.flat.copy_(torch.randn_like(red.flat) * 1e-2)
        try:
            opt = make_opt(form, [p for p in net.parameters()])
            for _ in range(20):
                opt.step()
        except (RuntimeError, ValueError, TypeError) as e:  # (a torch form this build does not have)
            if form.startswith("hip"):
                raise
            print("%s: not available here (%s)" % (form, str(e).splitlines()[0]))
            continue
        setups[form] = (net, red, opt)
    n_par = sum(p.numel() for p in setups["hip-sgd"][0].parameters())
    print("parameters: %d tensors, %d floats; traffic of one update: SGD with momentum and RMSprop 5 arrays = %.2f MB, Adam 7 = %.2f MB"
          % (len(list(setups["hip-sgd"][0].parameters())), n_par, 5 * 4 * n_par / 1e6, 7 * 4 * n_par / 1e6))
    for r in range(rounds):
        for form in setups:
            opt = setups[form][2]
            enq, comp = timed(lambda i: opt.step(), steps)
            print("round %d  %-22s enqueue %.4f ms   complete %.4f ms" % (r + 1, form, enq, comp))
    for form in setups:
        assert all(torch.isfinite(p).all() for p in setups[form][0].parameters()), form


def part2(steps, rounds):
    from samplenet_amd import optim
    from samplenet_amd.engine import SamplerTrainStep
    from samplenet_amd.parallel import FlatGradAllReducer

    print("part 2: the captured training step, B = %d, the update as its last node (%d steps per round, %d alternated rounds)"
          % (B, steps, rounds))
    gen = torch.Generator(device="cuda").manual_seed(1234)
    make = {"no-update": lambda ps: None, "adam": lambda ps: optim.Adam(ps, lr=1e-3),
            "sgd": lambda ps: optim.SGD(ps, lr=1e-3, momentum=0.9), "rmsprop": lambda ps: optim.RMSprop(ps, lr=1e-3)}
    variants = {}
    for name in LEGS:
        net = make_net()
        red = FlatGradAllReducer(net)
        pool = [torch.rand(B, N, 3, device="cuda", generator=gen) - 0.5 for _ in range(8)]
        st = SamplerTrainStep(net, pool[0], alpha=0.01, lmbda=0.01, gamma=1.0, delta=0.0, reducer=red, input_ring=pool,
                              optimizer=make[name](list(net.parameters())))
        assert len(st._ring_graphs[0]) == 1 and (name == "no-update" or st._update_in_graph())
        fn = lambda i, st=st: st.replay(i % 8)  # noqa: E731
        for i in range(50):
            fn(i)
        variants[name] = (fn, st, net)
    comp = {name: [] for name in LEGS}
    for r in range(rounds):
        for name in LEGS:
            enq, c = timed(variants[name][0], steps)
            comp[name].append(c)
            print("round %d  %-10s enqueue %.4f ms   complete %.4f ms   (%.0f clouds/s)" % (r + 1, name, enq, c, B / c * 1e3))
    for name, (fn, st, net) in variants.items():
        st.check()
        assert all(torch.isfinite(p).all() for p in net.parameters()), name
    print("summary (ms per step):")
    spread = max(max(v) - min(v) for v in comp.values())
    for name in LEGS:
        v = comp[name]
        print("  %-10s mean %.4f   range %.4f .. %.4f   (spread between its repeated legs %.4f)" % (name, sum(v) / len(v), min(v), max(v), max(v) - min(v)))
    inc = {}
    for name in LEGS[1:]:
        d = [a - b for a, b in zip(comp[name], comp["no-update"])]
        inc[name] = sum(d) / len(d)
        print("  increment of %-8s over no-update, round by round: mean %+.4f   range %+.4f .. %+.4f" % (name, inc[name], min(d), max(d)))
    print("  largest spread between repeated legs of one variant: %.4f" % spread)
    for name in ("sgd", "rmsprop"):
        over = inc[name] - inc["adam"]
        print("  %s increment minus adam increment: %+.4f -> %s" % (name, over, "EXCEEDS the spread" if over > spread else
                                                                      "does not exceed Adam's by more than the spread"))


def main():
    import argparse

    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_bench: needs a GPU (a CPU run measures nothing)")
    print("device:", torch.cuda.get_device_name(0), "| torch", torch.__version__)
    part1(args.steps, args.rounds)
    part2(args.steps, args.rounds)


if __name__ == "__main__":
    main()
