"""Build libsamplenet_hip.so (hand-written HIP for gfx950) in-tree with hipcc.

    python samplenet_amd/build.py            # incremental   (run as a script: importing the package needs the library)
    python samplenet_amd/build.py --force
    python samplenet_amd/build.py --variant NAME --unit FILE.hip[,FILE2.hip] [--flags "-D..."]   # build_variant: same-box A/B
    python samplenet_amd/build.py --timeline [--level 1|2] [--flags "-D..."]                     # build_timeline: phase stamps

hipcc cross-compiles without a GPU.  The shared object lands in samplenet_amd/lib/ so that it
travels with the source snapshot to the GPU box (it is git-ignored, not gpurun-ignored).
Variants land in tools/_ab/, which is kept out of history in the same way.
Every hipcc line of the library, the product's and a variant's, is assembled here: compile_command / link_command.
"""
import os
import shlex
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
OUT_DIR = os.path.join(HERE, "lib")
LIB = os.path.join(OUT_DIR, "libsamplenet_hip.so")
AB_DIR = os.path.join(ROOT, "tools", "_ab")
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
    # the per-point segmentation terms: the same contract (tests/seg_terms_ref.py counts from the order written in the file)
    ("seg_terms.hip", ["-ffp-contract=off"]),
    # the ball query's distance is difference, product, sum and one correctly rounded sqrt (tests/ball_ref.py restates it in fp32)
    ("ball_query.hip", ["-ffp-contract=off"]),
    # the three-NN distance is difference, product, sum in one written-out order (tests/interp_ref.py restates it in fp32)
    ("feature_propagate.hip", ["-ffp-contract=off"]),
    # the set abstraction's row-layout grouping shares the ball query's distance; its gradient and the group pool's partial sums
    # are written-out orders of rounded adds (tests/group_rows_ref.py restates them)
    ("set_abstraction.hip", ["-ffp-contract=off"]),
    # the feature propagation's row assembly, its gradient and the top BatchNorm's partial sums: written-out orders (tests/fp_rows_ref.py)
    ("feature_rows.hip", ["-ffp-contract=off"]),
]
# No COMPILER-GENERATED packed fp32 arithmetic (v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32) in device code: with a SECOND process on the same GPU
# (two ranks on one device, a monitoring job) kernels carrying the compiler's SLP-packed f32 ops returned wrong LOW halves in ~1 %
# of the launches on this platform (bit-exact statistics deviating in the even channels of the xyz layer;
# tools/cotenancy_stress.py reproduces it in seconds; 0 events in 16 000 passes without the packed ops, ~1 % slower step).
# The feature switch only means something to the device compile: the host compile reports it as unknown (filtered below).
NO_PACKED_F32 = ["-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"]
COMMON = ["-O3", "-std=c++17", "-fPIC", f"--offload-arch={ARCH}", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
          "-Wall", "-Wno-unused-function"] + NO_PACKED_F32
# SAMPLENET_AMD_EMD_SCALAR=1: the EMD sweeps without packed fp32 instructions (scalar pair helpers, bit-identical results, ~1.4x
# slower sweeps).  The flags come on top of emd.hip's own: the define, and the feature switch its "+packed" took away.
EMD_SCALAR = ("emd.hip", ["-DSN_EMD_SCALAR_F32=1"] + NO_PACKED_F32)
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


def compile_command(src, obj, extra=()):
    """argv that compiles `src` (a path) into `obj`: the common flags, the flags SOURCES gives a file of that name, then `extra`."""
    flags = dict(SOURCES).get(os.path.basename(src), []) + list(extra)
    common = COMMON
    if "+packed" in flags:
        flags = [f for f in flags if f != "+packed"]
        common = [f for f in COMMON if f not in NO_PACKED_F32]
    return [_hipcc(), "-x", "hip", "-c", src, "-o", obj] + common + flags


def link_command(out, objs):
    return [_hipcc(), "-shared", "-fPIC", f"--offload-arch={ARCH}", "-o", out] + list(objs)


def _product_objects():
    """{unit of SOURCES: (its object in the product build, extra flags)}, in SOURCES' order"""
    units = {src: (os.path.join(OUT_DIR, os.path.splitext(src)[0] + ".o"), []) for src, _ in SOURCES}
    if os.environ.get("SAMPLENET_AMD_EMD_SCALAR") == "1":
        # the object lands beside the default one under another name so the two never get mixed up
        units[EMD_SCALAR[0]] = (os.path.join(OUT_DIR, "emd_scalar.o"), EMD_SCALAR[1])
    return units


def _compile(jobs, verbose):
    """Run (label, argv) compiles side by side; hipcc's complaints go to stderr, a failure raises with the labels."""
    procs = []
    for label, cmd in jobs:
        if verbose:
            print(" ".join(cmd))
        procs.append((label, subprocess.Popen(cmd, stderr=subprocess.PIPE, text=True)))
    failed = []
    for label, p in procs:
        _, err = p.communicate()
        err = "\n".join(l for l in err.splitlines() if _HOST_NOISE not in l)
        if err.strip():
            sys.stderr.write(err + "\n")
        if p.returncode != 0:
            failed.append(label)
    if failed:
        raise RuntimeError("hipcc failed on " + ", ".join(failed))


def build(force=False, verbose=False):
    os.makedirs(OUT_DIR, exist_ok=True)
    headers = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    headers += [os.path.join(ROOT, "include", h) for h in ("samplenet_hip.h", "samplenet_hip_internal.h")]
    units = _product_objects()
    jobs = [(src, compile_command(os.path.join(CSRC, src), obj, extra)) for src, (obj, extra) in units.items()
            if force or _stale(obj, [os.path.join(CSRC, src)] + headers)]
    _compile(jobs, verbose)
    objs = [obj for obj, _ in units.values()]
    if jobs or force or _stale(LIB, objs):
        cmd = link_command(LIB, objs)
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
    return LIB


def variant_objects(name, remake, out_dir=AB_DIR, merge=()):
    """{unit of SOURCES: the object that carries it in variant `name`}, in SOURCES' order: out_dir/<stem>_<name>.o for a remade
    unit, the one object of merge[0] for every merged unit, the product build's object for the rest."""
    product = _product_objects()
    for unit in list(remake) + list(merge):
        if unit not in product:
            raise ValueError("%s is not a unit of build.SOURCES" % unit)

    def made(unit):
        return os.path.join(out_dir, "%s_%s.o" % (os.path.splitext(unit)[0], name))

    return {unit: made(merge[0]) if unit in merge else made(unit) if unit in remake else product[unit][0] for unit in product}


def merged_source(merge):
    """Text of the translation unit that compiles the units of `merge` as one."""
    return "".join('#include "%s"\n' % unit for unit in merge)


def build_variant(name, remake, out_dir=AB_DIR, merge=(), verbose=False):
    """A second build of the library, out_dir/libsamplenet_hip_<name>.so: the units `remake` names ({file name: extra flags}) compiled
    with those flags on top of their own, the units of `merge` compiled as ONE translation unit (the common flags and
    remake[merge[0]]), every other unit of SOURCES as the product build has it.  SAMPLENET_AMD_LIB=<that file> runs it."""
    objs = variant_objects(name, remake, out_dir, merge)
    build(verbose=verbose)
    os.makedirs(out_dir, exist_ok=True)
    jobs = [(unit, compile_command(os.path.join(CSRC, unit), objs[unit], extra)) for unit, extra in remake.items() if unit not in merge]
    if merge:
        tu = os.path.splitext(objs[merge[0]])[0] + ".hip"
        with open(tu, "w") as f:
            f.write(merged_source(merge))
        jobs.append((os.path.basename(tu), compile_command(tu, objs[merge[0]], remake.get(merge[0], []))))
    _compile(jobs, verbose)
    out = os.path.join(out_dir, "libsamplenet_hip_%s.so" % name)
    cmd = link_command(out, dict.fromkeys(objs.values()))
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return out


def build_timeline(level=1, flags=(), verbose=False):
    """The debug library with per-workgroup phase timestamps (tools/timeline.py and its kin: the MLP GEMM kernels;
    tools/pairscan_timeline.py: the pair scan and the loss backward).  The four MLP units compile as ONE, so that the stamp buffers of
    mlp_device.h exist once, whichever kernel writes them; `flags` go to that unit.  level 2: every stamp of the geometric kernels
    first waits for the memory operations before it (serialised phases); 1: stamps only."""
    mlp = ("pointnet_mlp.hip", "pointnet_mlp_backward.hip", "fc_chain.hip", "task_network.hip")
    geo = ["-DSN_PS_TIMELINE=%d" % level, "-DSN_CS_TIMELINE=%d" % level]
    remake = {mlp[0]: ["-DSN_TIMELINE"] + list(flags), "capi_common.cpp": ["-DSN_TIMELINE"], "pairscan.hip": geo, "sampler_step_loss.hip": geo}
    return build_variant("tl", remake, merge=mlp, verbose=verbose)


def _main(argv):
    def value(option, default=""):
        return argv[argv.index(option) + 1] if option in argv else default

    flags = shlex.split(value("--flags"))
    if "--timeline" in argv:
        return build_timeline(int(value("--level", "1")), flags, verbose=True)
    if "--variant" in argv:
        return build_variant(value("--variant"), {unit: flags for unit in value("--unit").split(",")}, verbose=True)
    return build(force="--force" in argv, verbose=True)


if __name__ == "__main__":
    print(_main(sys.argv[1:]))
