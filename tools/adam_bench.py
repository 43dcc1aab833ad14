"""What the optimizer update costs behind the sampler's training step, on the sampler's real parameter set (the headline
configuration of bench.py: B = 32, N = 1024, M = 64, K = 8; ~30 tensors, 249,793 floats).

    python tools/adam_bench.py > profiles/adam/adam_bench.txt

Part 1 -- the update alone, gradients resident in the reducer's bucket: samplenet_amd.optim.Adam (one launch) against torch.optim.Adam
in its default, foreach=True and fused=True forms.  Per form:
    enqueue   host time per step() with the device left to drain on its own (a host clock around the calls, no synchronise inside)
    complete  host clock around the same number of calls ENDING in a synchronise: what a training loop pays per step -- the larger of
              the host's launch path and the device's work
    graph     (ours only) the update captured 50 times in one graph and replayed: device time per update without any host launch
Part 2 -- the captured training step (engine.SamplerTrainStep on an 8-entry input ring, as bench.py runs it) with the update as a node
of its graph, against the same captured step followed by each form's step() from Python, and against the step without any update.
Three alternated rounds per variant; every figure is milliseconds per step, to completion.
"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, N, M, K = 32, 1024, 64, 8
FORMS = ("hip", "torch-default", "torch-foreach", "torch-fused")


def make_net():
    from samplenet_amd import SampleNet

    torch.manual_seed(0)
    return SampleNet(M, 128, group_size=K, initial_temperature=1.0, is_temperature_trainable=True, min_sigma=1e-2,
                     input_shape="bnc", output_shape="bnc").cuda().train()


def make_opt(form, params):
    from samplenet_amd.optim import Adam

    if form == "hip":
        return Adam(params, lr=1e-3)
    kw = {"torch-default": {}, "torch-foreach": {"foreach": True}, "torch-fused": {"fused": True}}[form]
    return torch.optim.Adam(params, lr=1e-3, **kw)


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

    print("part 1: the update alone (%d steps per round, %d alternated rounds)" % (steps, rounds))
    setups = {}
    for form in FORMS:
        net = make_net()
        red = FlatGradAllReducer(net)
        red.flat.copy_(torch.randn_like(red.flat) * 1e-2)
        opt = make_opt(form, [p for p in net.parameters()])
        for _ in range(20):
            opt.step()
        setups[form] = (net, red, opt)
    n_par = sum(p.numel() for p in setups["hip"][0].parameters())
    print("parameters: %d tensors, %d floats; traffic of one update (read p, g, m, v; write p, m, v): %.2f MB"
          % (len(list(setups["hip"][0].parameters())), n_par, 7 * 4 * n_par / 1e6))
    for r in range(rounds):
        for form in FORMS:
            opt = setups[form][2]
            enq, comp = timed(lambda i: opt.step(), steps)
            print("round %d  %-14s enqueue %.4f ms   complete %.4f ms" % (r + 1, form, enq, comp))
    opt = setups["hip"][2]
    opt.prepare()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(50):
            opt._launch()
    for r in range(rounds):
        _, comp = timed(lambda i: g.replay(), 40)
        print("round %d  %-14s graph of 50 updates: %.4f ms per update (device time, no host launch)" % (r + 1, "hip", comp / 50))


def part2(steps, rounds):
    from samplenet_amd.engine import SamplerTrainStep
    from samplenet_amd.parallel import FlatGradAllReducer

    print("part 2: the captured training step, B = %d (%d steps per round, %d alternated rounds)" % (B, steps, rounds))
    gen = torch.Generator(device="cuda").manual_seed(1234)
    variants = {}
    for name in ("no-update", "hip-in-graph") + tuple("step+" + f for f in FORMS):
        net = make_net()
        red = FlatGradAllReducer(net)
        pool = [torch.rand(B, N, 3, device="cuda", generator=gen) - 0.5 for _ in range(8)]
        opt = None if name == "no-update" else make_opt("hip" if name == "hip-in-graph" else name[5:], list(net.parameters()))
        st = SamplerTrainStep(net, pool[0], alpha=0.01, lmbda=0.01, gamma=1.0, delta=0.0, reducer=red, input_ring=pool,
                              optimizer=opt if name == "hip-in-graph" else None)
        if name in ("no-update", "hip-in-graph"):
            fn = lambda i, st=st: st.replay(i % 8)  # noqa: E731
        else:
            def fn(i, st=st, opt=opt):
                st.replay(i % 8)
                opt.step()
        for i in range(50):
            fn(i)
        variants[name] = (fn, st, net, opt)
    launches = {n: len(v[1]._ring_graphs[0]) for n, v in variants.items()}
    assert all(c == 1 for c in launches.values())
    for r in range(rounds):
        for name, (fn, st, net, opt) in variants.items():
            enq, comp = timed(fn, steps)
            print("round %d  %-20s enqueue %.4f ms   complete %.4f ms   (%.0f clouds/s)" % (r + 1, name, enq, comp, B / comp * 1e3))
    for name, (fn, st, net, opt) in variants.items():
        st.check()
        assert all(torch.isfinite(p).all() for p in net.parameters()), name


def main():
    import argparse

    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("adam_bench: needs a GPU (a CPU run measures nothing)")
    print("device:", torch.cuda.get_device_name(0), "| torch", torch.__version__)
    part1(args.steps, args.rounds)
    part2(args.steps, args.rounds)


if __name__ == "__main__":
    main()
