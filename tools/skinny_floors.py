"""Measures the floor tests/test_gpu_skinny.py's real-data test uses: the worst |fp32 - fp64| / A, element by element, of torch's own
fp32 F.linear over that test's data (three seeds, R in {5, 33, 128}, both layouts, gated + ReLU and plain), per shape and per K class
(K <= 64, <= 1024, > 1024).  The constants come from the torch column alone; the library's own worst ratios on the same data stand
beside them for the record.

    python tools/skinny_floors.py > profiles/skinny/floors.txt
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import skinny_ref as S  # noqa: E402
import test_gpu_skinny as T  # noqa: E402

if __name__ == "__main__":
    print("device:", torch.cuda.get_device_name(0), "| torch", torch.__version__, "| 3 seeds x R in (5, 33, 128) x 2 layouts x 2 variants per shape")
    print("    ratio = max over elements of |got - fp64| / (|x . mask| |W|^T + |b|)")
    floors, ours = [0.0] * 3, [0.0] * 3
    for shape in S.SHAPES:
        K, N = shape
        t = max(T.real_ratios(shape, route="torch").values())
        l = max(T.real_ratios(shape, route="library").values())
        c = S.k_class(K)
        floors[c], ours[c] = max(floors[c], t), max(ours[c], l)
        print("    (%4d, %4d)  torch fp32 F.linear %.3e   library %.3e   ceiling (K + 8) 2^-24 %.3e" % (K, N, t, l, (K + 8) * 2.0 ** -24))
    for c, name in enumerate(("K <= 64", "K <= 1024", "K > 1024")):
        print("    class %-9s  -> torch floor %.3e  (bar = 4 x floor = %.3e)   library worst %.3e" % (name, floors[c], 4 * floors[c], ours[c]))
