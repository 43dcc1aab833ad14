"""The library for the host tests: samplenet_amd/build.py loaded by path (importing the package needs the library to exist
already) and the product build made where it is missing -- hipcc cross-compiles gfx950 without a GPU."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_build():
    spec = importlib.util.spec_from_file_location("sn_build", os.path.join(ROOT, "samplenet_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def ensure_built():
    """Path of libsamplenet_hip.so, built first if it is not there."""
    build = load_build()
    if not os.path.exists(build.LIB):
        build.build()
    return build.LIB
