"""Host-side tests of samplenet_amd/build.py's recipe (no GPU): every hipcc line of the library, the product's and a variant's, comes
from compile_command / link_command over the one list SOURCES, so a variant is complete by construction and carries the product's flags."""
import ctypes
import os

import pytest

from built_lib import load_build

build = load_build()


def _after(argv, first, then):
    """Every flag of `then` stands behind every flag of `first`."""
    return all(f in argv for f in first + then) and max(map(argv.index, first), default=-1) < min(map(argv.index, then))


def test_compile_command_carries_each_units_flags_and_the_packed_fp32_switch():
    """Pinned to structure, not to a copy of the list: the target, both include directories and the unit's own flags on every line;
    the packed-fp32 switch on all of them but emd.hip (hand-written packed instructions: the compiler's own packing is off through
    the SLP vectoriser instead); extra flags behind the unit's own, so that they win."""
    assert len(build.SOURCES) == len(dict(build.SOURCES)) >= 24
    switch = " ".join(build.NO_PACKED_F32)
    for src, flags in build.SOURCES:
        path = os.path.join(build.CSRC, src)
        assert os.path.exists(path), src
        argv = build.compile_command(path, "/tmp/x.o", extra=["-DEXTRA=1", "-O1"])
        assert argv[1:6] == ["-x", "hip", "-c", path, "-o"] and argv[6] == "/tmp/x.o", src
        for flag in ("--offload-arch=gfx950", "-I" + os.path.join(build.ROOT, "include"), "-I" + build.CSRC):
            assert argv.count(flag) == 1, (src, flag)
        own = [f for f in flags if f != "+packed"]
        assert _after(argv, ["-O3"], own + ["-DEXTRA=1"]) and _after(argv, ["-O3"] + own, ["-DEXTRA=1", "-O1"]), src
        assert "+packed" not in argv
        if src == "emd.hip":
            assert switch not in " ".join(argv) and "-fno-slp-vectorize" in argv
        else:
            assert switch in " ".join(argv), src
    # a file that is no unit of the library: the common flags alone (the switch among them), then the extra ones
    argv = build.compile_command("/tmp/merged_tl.hip", "/tmp/m.o", extra=["-DX"])
    assert switch in " ".join(argv) and "-ffp-contract=off" not in argv and argv[-1] == "-DX"
    # the EMD scalar switch is data on top of emd.hip's own flags: its define, and the feature switch back on
    argv = build.compile_command(os.path.join(build.CSRC, build.EMD_SCALAR[0]), "/tmp/e.o", extra=build.EMD_SCALAR[1])
    assert switch in " ".join(argv) and "-DSN_EMD_SCALAR_F32=1" in argv and "-fno-slp-vectorize" in argv


def test_a_variant_exports_the_whole_abi(tmp_path):
    """One small unit remade with a flag of its own, every other unit from the product build: the variant binds every prototype of
    both headers (what `import samplenet_amd` asks of SAMPLENET_AMD_LIB), and is linked from one object per unit of SOURCES."""
    import torch  # noqa: F401  (its bundled HIP runtime satisfies the library's libamdhip64 dependency)

    remake = {"nn_matching.hip": ["-DSN_TEST_VARIANT=1"]}
    so = build.build_variant("t", remake, out_dir=str(tmp_path))
    assert so == str(tmp_path / "libsamplenet_hip_t.so") and os.path.exists(so)
    objs = build.variant_objects("t", remake, out_dir=str(tmp_path))
    assert list(objs) == [src for src, _ in build.SOURCES]
    assert objs.pop("nn_matching.hip") == str(tmp_path / "nn_matching_t.o")
    assert all(obj == os.path.join(build.OUT_DIR, os.path.splitext(src)[0] + ".o") for src, obj in objs.items())

    from samplenet_amd._lib import PROTOTYPES, bind

    lib = bind(ctypes.CDLL(so))
    assert len(PROTOTYPES) >= 30 and lib.sn_abi_version() == 1


def test_a_unit_outside_sources_is_refused(tmp_path):
    for kwargs in ({"remake": {"geometry_ops.hip": []}}, {"remake": {}, "merge": ("pointnet_mlp.hip", "geometry_ops.hip")}):
        with pytest.raises(ValueError, match=r"geometry_ops\.hip is not a unit of build\.SOURCES"):
            build.build_variant("t", out_dir=str(tmp_path), **kwargs)
    assert not os.listdir(tmp_path)


def test_merged_units_are_one_translation_unit_of_includes(tmp_path):
    """The text only (compiling the timeline's merged unit takes minutes): one #include per merged unit, in order; and the merged
    units share ONE object, named for the first, so the link still holds each unit once."""
    merge = ("pointnet_mlp.hip", "pointnet_mlp_backward.hip", "fc_chain.hip", "task_network.hip")
    assert build.merged_source(merge) == "".join('#include "%s"\n' % unit for unit in merge)
    assert build.merged_source(merge[::-1]).splitlines()[0] == '#include "task_network.hip"'
    objs = build.variant_objects("tl", {merge[0]: ["-DSN_TIMELINE"], "pairscan.hip": []}, out_dir=str(tmp_path), merge=merge)
    assert {objs[unit] for unit in merge} == {str(tmp_path / "pointnet_mlp_tl.o")}
    assert objs["pairscan.hip"] == str(tmp_path / "pairscan_tl.o")
    assert len(set(objs.values())) == len(build.SOURCES) - len(merge) + 1
