"""Worst error of the device's logf / sqrtf / sincosf over all 2^24 inputs the batch assembly's draws can produce, in ulps of the
result -- the figures tests/test_gpu_batch_assemble.py charges each library call (LIB_ULPS; the test uses twice the measured worst).

    python tools/batch_floors.py        # builds tools/micro/batch_floors(.hip) if needed, runs it, writes profiles/input/floors.txt
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "micro", "batch_floors.hip")
EXE = os.path.join(ROOT, "tools", "micro", "batch_floors")


def main():
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < os.path.getmtime(SRC):
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        subprocess.check_call([hipcc, "-O3", "--offload-arch=gfx950", "-ffp-contract=off", SRC, "-o", EXE])
    out = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    if out.returncode != 0:
        sys.exit("batch_floors failed: %s" % out.stderr[-500:])
    vals = dict(line.split() for line in out.stdout.splitlines() if line.strip())
    import torch

    text = ["# Worst |fp32 library call - fp64| in ulps of the true result (1 ulp = 2^-23 |true|), exhaustive over the 2^24 inputs the draws of",
            "# sn_batch_assemble can produce (tools/micro/batch_floors.hip).  Measured by tools/batch_floors.py on %s, HIP %s." %
            (torch.cuda.get_device_name(0), torch.version.hip),
            "# tests/test_gpu_batch_assemble.py: LIB_ULPS holds these three figures; the bar charges twice each."]
    text += ["%s %s" % (k, vals[k]) for k in ("logf", "sqrtf", "sincosf")]
    path = os.path.join(ROOT, "profiles", "input", "floors.txt")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(text) + "\n")
    print("\n".join(text))


if __name__ == "__main__":
    main()
