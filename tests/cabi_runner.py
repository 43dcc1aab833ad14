"""The runner the argument-table tests share (test_cabi_arguments.py, test_ball_host.py, test_interp_host.py): a table of
(id, entry, arguments, expected code, text the message must contain | None) is walked once by one child process that sees no
GPU, so that a call that slipped through a missing check comes back as an error code instead of touching a device with the
made-up pointers.  Arguments are JSON values; these stand for pointers:
    "PTR"    a non-NULL (never dereferenced) device pointer
    "HOSTI"  a real host int array {4}
    "HOSTP"  a real host array of ONE non-NULL (never dereferenced) device pointer
    ["HOSTI", v0, v1, ...] / ["HOSTP", p0, p1, ...]   the same with the values spelled out (a pointer of 0 is NULL)"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = r"""
import ctypes, json, sys
sys.path.insert(0, %r)
from samplenet_amd._lib import lib
cases = json.load(sys.stdin)
host = (ctypes.c_int * 1)(4)
hostp = (ctypes.c_void_p * 1)(4096)
def host_array(a):  # ["HOSTI", ints...] / ["HOSTP", addresses...; 0 = NULL]
    ty = ctypes.c_int if a[0] == "HOSTI" else ctypes.c_void_p
    return (ty * (len(a) - 1))(*[(v or None) if a[0] == "HOSTP" else v for v in a[1:]])
res = []
for cid, name, args, _, _ in cases:
    keep = [host_array(a) if isinstance(a, list) else a for a in args]
    conv = [ctypes.c_void_p(4096) if a == "PTR" else (ctypes.cast(host, ctypes.c_void_p) if a == "HOSTI" else
            (ctypes.cast(hostp, ctypes.c_void_p) if a == "HOSTP" else (ctypes.cast(a, ctypes.c_void_p) if isinstance(a, ctypes.Array) else a)))
            for a in keep]
    rc = getattr(lib, name)(*conv)
    res.append([cid, int(rc), (lib.sn_last_error_string() or b"").decode()])
print("RESULTS " + json.dumps(res))
"""


def run_cases(cases):
    """{id: (return code, sn_last_error_string() after the call)} of every case"""
    env = dict(os.environ)
    env.update(HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")  # argument checks need no device: none is offered
    p = subprocess.run([sys.executable, "-c", _CHILD % ROOT], input=json.dumps(cases), capture_output=True, text=True, env=env,
                       timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULTS ")][-1]
    return {cid: (rc, msg) for cid, rc, msg in json.loads(line[len("RESULTS "):])}


def check_case(results, case):
    cid, name, args, want, text = case
    rc, msg = results[cid]
    assert rc == want, (cid, rc, msg)
    if text is not None:
        assert text in msg, (cid, msg)
        assert msg.startswith(name + ":"), (cid, msg)  # the entry's own name, not that of a shared implementation
