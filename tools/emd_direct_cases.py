"""profiles/emd_direct/cases.txt: per admitted case of tests/emd_ref.py the distances from float64 that the two test files print.

    python -m pytest tests/test_emd_host.py -q -s -k "admitted" > host.log           # no GPU
    python -m pytest tests/test_gpu_emd_direct.py -q -s -m gpu > device.log          # MI355X
    python tools/emd_direct_cases.py host.log device.log > profiles/emd_direct/cases.txt

Regenerate whenever a seed in tests/emd_ref.py changes: the case names carry the seed, and a case missing from either log is an error."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import emd_ref as E  # noqa: E402

CASE = r"\.*(\d+x\d+x\d+-\w+-s\d+) "
DEVICE = ("sn_approxmatch", "sn_emd_loss seg=1 2d=1", "sn_emd_loss_fast seg=1 2d=1", "sn_emd_loss_fast seg=1 2d=0", "sn_emd_loss_fast seg=0 2d=1")


def main(host_log, device_log):
    cpu, dev = {}, {}
    for line in open(host_log):
        m = re.match(CASE + r"(oracle|fast model)\s+(.*)", line.strip())
        if m:
            cpu.setdefault(m.group(1), {})[m.group(2)] = m.group(3)
    for line in open(device_log):
        m = re.match(CASE + "(" + "|".join(DEVICE) + r")\s+(.*)", line.strip())
        if m:
            dev.setdefault(m.group(1), {})[m.group(2)] = m.group(3)
        m = re.match(CASE + r"vs oracle: (.*)", line.strip())
        if m:
            dev.setdefault(m.group(1), {})["vs oracle"] = m.group(2)
    print("Admitted cases of tests/emd_ref.py (b x n x m - recipe - seed): distance from the float64 reference of the fp32 oracle (its")
    print("  ratioR / ratioL figures: the plain float32 numpy evaluation's) and of the fast-exponential model (cpu: tests/test_emd_host.py),")
    print("  and of the device entries (gpu: MI355X, tests/test_gpu_emd_direct.py; `seg`: sn_emd_set_segments, `2d`: sn_emd_set_sweep2d).")
    print("  Figures as tests/emd_ref.py figures() scales them.  Bars: match 5e-4, match mean 1e-7, cost 1e-5, grad max 5e-3, grad norm 1e-4,")
    print("  ratioR and ratioL held 5e-4 multiL multiR, ratios as match 5e-4.  Regenerate: tools/emd_direct_cases.py (its header says how).")
    print()
    for c in E.cases():
        k = E.case_id(c)
        if k not in cpu or k not in dev:
            raise SystemExit("case %s is missing from a log" % k)
        print(k)
        for src, d in (("cpu", cpu[k]), ("gpu", dev[k])):
            for name, v in d.items():
                print("    %s %-28s %s" % (src, name, v))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
