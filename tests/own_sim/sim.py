"""Build the host harness of the context's owners (svjedi-graph_amd/csrc/svjg_own.h; tests only)."""
import os

from tests import sim_build

HERE = os.path.dirname(os.path.abspath(__file__))
MAIN = os.path.join(HERE, "_own_sim_main")
ROCM_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")


def build_main():
    """the stand-alone program under AddressSanitizer and UBSan (its own main and its own stand-ins of the HIP calls: no HIP runtime is linked,
    nothing is preloaded into anything)"""
    return sim_build.program(MAIN, os.path.join(HERE, "own_sim.cpp"), [os.path.join(HERE, "..", "..", "svjedi-graph_amd", "csrc", "svjg_own.h")],
                             ["__HIP_PLATFORM_AMD__"], extra=["-I" + ROCM_INCLUDE])
