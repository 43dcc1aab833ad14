"""Build libsamplenet_hip.so (hand-written HIP for gfx950) in-tree with hipcc.

    python samplenet_amd/build.py            # incremental   (run as a script: importing the package needs the library)
    python samplenet_amd/build.py --force

hipcc cross-compiles without a GPU.  The shared object lands in samplenet_amd/lib/ so that it
travels with the source snapshot to the GPU box (it is git-ignored, not gpurun-ignored).
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
OUT_DIR = os.path.join(HERE, "lib")
LIB = os.path.join(OUT_DIR, "libsamplenet_hip.so")
ARCH = "gfx950"

# (source, extra flags).  The geometric kernels must round like the reference's CPU code
# (product then sum, never FMA): -ffp-contract=off on top of the in-source pragma.
SOURCES = [
    ("capi_common.cpp", []),
    ("pairscan.hip", ["-ffp-contract=off"]),
    # the Chamfer backward and the losses on it add the owners' terms in the reference's order (chamfer_owner.h: owner_sum)
    ("chamfer_backward.hip", ["-ffp-contract=off"]),
    # SoftProjection's backward (soft_query.h) and the gather / group ops with their ordered index-add
    ("soft_projection.hip", ["-ffp-contract=off"]),
    # the sampler step's fused loss: Chamfer and soft-projection backward of a query in one launch, the step tail, the surface values
    ("sampler_step_loss.hip", ["-ffp-contract=off"]),
    # PCRNet's output head and the quaternion rotation, apart and fused
    ("pcrnet_head.hip", ["-ffp-contract=off"]),
    # inference matching: numpy's fp64 distance, product then sum
    ("nn_matching.hip", ["-ffp-contract=off"]),
    # the progressive sampler's prefix minima, pack / pad ops and fused loss: the Chamfer scan's expression and tie rule
    ("progressive_prefix.hip", ["-ffp-contract=off"]),
    ("sampling.hip", ["-ffp-contract=off"]),
    # the ranking's fp64 distance is numpy's: product then sum, one rounding per operation (tests/rank_ref.py)
    ("rank_points.hip", ["-ffp-contract=off"]),
    # the retrieval distance is difference, product, sum in one written-out order (tests/retrieval_ref.py restates it in fp32)
    ("retrieval.hip", ["-ffp-contract=off"]),
    # emd.hip carries HAND-WRITTEN packed fp32 instructions (inline asm, destination pair disjoint from every source: the form a
    # replayed instruction cannot get wrong) -- the assembler needs the feature, the compiler's own packing stays off through
    # the SLP vectoriser switch; tests/test_cabi_and_host.py checks the disassembly for both properties
    ("emd.hip", ["-ffp-contract=off", "-fno-slp-vectorize", "+packed"]),
    ("pointnet_mlp.hip", []),
    ("pointnet_mlp_backward.hip", []),
    ("fc_chain.hip", []),
    ("task_network.hip", []),
    ("cloud_transform.hip", []),
    # the Adam / SGD / RMSprop updates' operation order is pinned (rounding bounds are derived from it): only the fmaf's written out
    ("optimizer.hip", ["-ffp-contract=off"]),
    # the batch assembly's fp32 operation order is its contract (include/samplenet_hip_internal.h; tests/batch_ref.py counts it)
    ("batch_assemble.hip", ["-ffp-contract=off"]),
    # the pose-error terms: every sum's order is written out (tests/pose_ref.py counts the roundings)
    ("pose_terms.hip", ["-ffp-contract=off"]),
    # the classification terms: the same contract (tests/cls_terms_ref.py counts from the order written in the file)
    ("cls_terms.hip", ["-ffp-contract=off"]),
    # the ball query's distance is difference, product, sum and one correctly rounded sqrt (tests/ball_ref.py restates it in fp32)
    ("ball_query.hip", ["-ffp-contract=off"]),
    # the three-NN distance is difference, product, sum in one written-out order (tests/interp_ref.py restates it in fp32)
    ("feature_propagate.hip", ["-ffp-contract=off"]),
    # the set abstraction's row-layout grouping shares the ball query's distance; its gradient and the group pool's partial sums
    # are written-out orders of rounded adds (tests/group_rows_ref.py restates them)
    ("set_abstraction.hip", ["-ffp-contract=off"]),
]
# No COMPILER-GENERATED packed fp32 arithmetic (v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32) in device code: with a SECOND process on the same GPU
# (two ranks on one device, a monitoring job) kernels carrying the compiler's SLP-packed f32 ops returned wrong LOW halves in ~1 %
# of the launches on this platform (bit-exact statistics deviating in the even channels of the xyz layer;
# tools/cotenancy_stress.py reproduces it in seconds; 0 events in 16 000 passes without the packed ops, ~1 % slower step).
# The feature switch only means something to the device compile: the host compile reports it as unknown (filtered below).
NO_PACKED_F32 = ["-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"]
COMMON = ["-O3", "-std=c++17", "-fPIC", f"--offload-arch={ARCH}", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
          "-Wall", "-Wno-unused-function"] + NO_PACKED_F32
_HOST_NOISE = "'-packed-fp32-ops' is not a recognized feature for this target"


def _hipcc():
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if cand and (os.path.isabs(cand) and os.path.exists(cand) or not os.path.isabs(cand)):
            return cand
    raise RuntimeError("hipcc not found")


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps if os.path.exists(d))


def build(force=False, verbose=False):
    os.makedirs(OUT_DIR, exist_ok=True)
    hipcc = _hipcc()
    headers = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    headers += [os.path.join(ROOT, "include", h) for h in ("samplenet_hip.h", "samplenet_hip_internal.h")]
    objs, jobs = [], []
    for src, extra in SOURCES:
        path = os.path.join(CSRC, src)
        if not os.path.exists(path):
            continue
        obj = os.path.join(OUT_DIR, os.path.splitext(src)[0] + ".o")
        objs.append(obj)
        if src == "emd.hip" and os.environ.get("SAMPLENET_AMD_EMD_SCALAR") == "1":
            # build switch: the EMD sweeps without packed fp32 instructions (scalar pair helpers, bit-identical results, ~1.4x
            # slower sweeps); the object lands beside the default one under another name so the two never get mixed up
            extra = ["-ffp-contract=off", "-fno-slp-vectorize", "-DSN_EMD_SCALAR_F32=1"]
            obj = os.path.join(OUT_DIR, "emd_scalar.o")
            objs[-1] = obj
        if force or _stale(obj, [path] + headers):
            common = COMMON
            if "+packed" in extra:
                extra = [f for f in extra if f != "+packed"]
                common = [f for f in COMMON if f not in NO_PACKED_F32]
            cmd = [hipcc, "-x", "hip", "-c", path, "-o", obj] + common + extra
            if verbose:
                print(" ".join(cmd))
            jobs.append((src, subprocess.Popen(cmd, stderr=subprocess.PIPE, text=True)))  # the units compile side by side
    failed = []
    for src, p in jobs:
        _, err = p.communicate()
        err = "\n".join(l for l in err.splitlines() if _HOST_NOISE not in l)
        if err.strip():
            sys.stderr.write(err + "\n")
        if p.returncode != 0:
            failed.append(src)
    if failed:
        raise RuntimeError("hipcc failed on " + ", ".join(failed))
    rebuilt = bool(jobs)
    if rebuilt or force or _stale(LIB, objs):
        cmd = [hipcc, "-shared", "-fPIC", f"--offload-arch={ARCH}", "-o", LIB] + objs
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
