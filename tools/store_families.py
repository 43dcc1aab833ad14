"""python tools/store_families.py DIR [NAME ...]: the store-policy experiment (mlp_device.h: SN_ST_Z / SN_ST_DY / SN_ST_PART) read out of
rocprofv3 kernel traces of the headline, one per variant library: DIR/kernel_stats_NAME.csv (+ DIR/trace_bench_NAME.json, the bench
line of the traced run).  One line per variant: avg us of the eight conv-stack GEMM kernels and of post_bwd_in3_kernel, and the sums a
family is judged on -- its writer kernels plus the kernel that reads what it writes:
  Z     the four forward GEMMs (each layer reads the Z of the one below)
  DY    the four backward GEMMs (each layer reads the dY of the one above)
  PART  the four backward GEMMs + post_bwd_in3_kernel (the reader of every weight-gradient / statistics partial)."""
import csv
import json
import os
import sys

KERNELS = [  # (label, substrings that must all occur in the kernel's name)
    ("f3-64-64", ("linear_fwd_kernel<sn::Tile<64, 64, 2, 2>", "true, true>")),
    ("f64-64", ("linear_fwd_kernel<sn::Tile<64, 64, 2, 2>", "true, false>")),
    ("f64-128", ("linear_fwd_kernel<sn::Tile<64, 128, 2, 4>, true, 2, 64,",)),
    ("f128-128", ("linear_fwd_kernel<sn::Tile<64, 128, 2, 4>, true, 2, 128,",)),
    ("b128x128", ("conv_bwd_bx3_kernel<128, 128,",)),
    ("b64-128", ("conv_bwd_bx3_kernel<64, 128,",)),
    ("b64x64", ("conv_bwd_bx3_kernel<64, 64, 1, true, false,",)),
    ("b64x64in3", ("conv_bwd_bx3_kernel<64, 64, 1, true, true,",)),
    ("post", ("post_bwd_in3_kernel",)),
]


def read(d, name):
    avg = {}
    with open(os.path.join(d, "kernel_stats_%s.csv" % name)) as f:
        for r in csv.DictReader(f):
            for label, keys in KERNELS:
                if all(k in r["Name"] for k in keys):
                    avg[label] = float(r["AverageNs"]) / 1e3
    ms = None
    p = os.path.join(d, "trace_bench_%s.json" % name)
    if os.path.exists(p):
        with open(p) as f:
            ms = json.load(f).get("ms_per_step")
    return avg, ms


def main():
    d = sys.argv[1]
    names = sys.argv[2:] or sorted(f[len("kernel_stats_"):-4] for f in os.listdir(d) if f.startswith("kernel_stats_") and f.endswith(".csv"))
    labels = [k for k, _ in KERNELS]
    print("# avg us per launch (rocprofv3 --kernel-trace --stats, bench.py --gpus 1 --no-probes); ms/step of the traced run")
    print("%-10s " % "variant" + " ".join("%9s" % k for k in labels) + "   fwd4=Z   bwd4=DY  bwd4+post=PART   all9   ms/step")
    for n in names:
        a, ms = read(d, n)
        fwd = sum(a[k] for k in labels[:4])
        bwd = sum(a[k] for k in labels[4:8])
        print("%-10s " % n + " ".join("%9.2f" % a[k] for k in labels) + " %8.2f %9.2f %15.2f %6.2f   %s" % (
            fwd, bwd, bwd + a["post"], fwd + bwd + a["post"], "%.4f" % ms if ms else "-"))


if __name__ == "__main__":
    main()
