"""The owners svjg_ctx is built from (svjedi-graph_amd/csrc/svjg_own.h), compiled with g++ against malloc-backed stand-ins of the HIP calls
(tests/own_sim): growth with and without the contents kept, every failure path of a reserve, release, moves, destruction order, pinned blocks."""
import os
import subprocess
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from tests.own_sim import sim                        # noqa: E402


def test_harness_under_the_sanitizers():
    """the stand-alone program (its own main) built with -fsanitize=address,undefined: exit 0, every check held, nothing alive at exit"""
    p = subprocess.run([sim.build_main()], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.startswith("own_sim ok:"), p.stdout + p.stderr
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr and "LeakSanitizer" not in p.stderr
