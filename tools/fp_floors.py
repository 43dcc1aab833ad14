"""Measures the floors tests/test_gpu_fp_module.py uses: per level and mode the worst error of torch's own fp32 evaluation of the
feature-propagation module (fused=False: torch weights, three_interpolate, cat, Conv2d, BatchNorm2d, ReLU) against float64, over 16
seeds, for every quantity the test compares.  The fused route takes no part: the indices come from ops.three_nn, everything else
is torch.

    python tools/fp_floors.py > profiles/fp_rows/floors.txt
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_fp_module as T  # noqa: E402

SEEDS = 16


if __name__ == "__main__":
    print("device:", torch.cuda.get_device_name(0), "| torch", torch.__version__, "| %d seeds per level and mode" % SEEDS)
    print("worst error of torch fp32 against float64 per quantity kind (a gradient: norm of the difference / norm of the float64 gradient; "
          "anything else: the largest element); FLOORS of tests/test_gpu_fp_module.py are these lines")
    for level in T.LEVELS:
        for mode in ("train", "eval"):
            worst = {}
            for seed in range(SEEDS):
                t32 = T.run(T.fresh_module(level, mode, seed), level, fused=False, seed=seed)
                idx, filled = T.kernel_idx(level, seed)
                ref, _ = T.float64_reference(T.fresh_module(level, mode, seed), level, idx, filled, seed=seed)
                for name, t in t32.items():
                    if not name.endswith("num_batches_tracked"):
                        k = T.quantity_kind(name)
                        worst[k] = max(worst.get(k, 0.0), T._err(t, ref[name], name))
            print("    %-11s %-5s  " % (level, mode) + "  ".join("%s %.2e" % kv for kv in worst.items()))
