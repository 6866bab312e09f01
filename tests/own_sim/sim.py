"""Build the host harness of the context's owners (svjedi-graph_amd/csrc/svjg_own.h; tests only)."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
MAIN = os.path.join(HERE, "_own_sim_main")
SRC = [os.path.join(HERE, "own_sim.cpp"), os.path.join(HERE, "..", "..", "svjedi-graph_amd", "csrc", "svjg_own.h")]
ROCM_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")


def build_main():
    """the stand-alone program under AddressSanitizer and UBSan (its own main and its own stand-ins of the HIP calls: no HIP runtime is linked,
    nothing is preloaded into anything)"""
    if not os.path.exists(MAIN) or os.path.getmtime(MAIN) < max(os.path.getmtime(s) for s in SRC):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + ROCM_INCLUDE, "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-o", MAIN, SRC[0]], check=True)
    return MAIN
