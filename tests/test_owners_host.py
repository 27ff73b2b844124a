"""The owning buffer types of csrc/mdns_internal.h checked on the host alone: tests/owners_host.cpp is a stand-alone
program (its own ``main``, the allocation seam over ``malloc`` with a live-block count and a failing call on demand),
built here with the address and undefined-behaviour sanitizers and run directly.  What it asserts: ``make`` is exact and
``fit`` keeps its growth policy, a failed allocation leaves an empty buffer, moves free the target's old block once, a
lazily made group of blocks is whole or absent whichever of its calls fails, and nothing is live at the end."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")


def test_owners_on_the_host(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "owners_host")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",         # (the runtimes inside the program: nothing to preload)
           "-D__HIP_PLATFORM_AMD__", "-I" + ROCM_INCLUDE, "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "massivedatans_amd", "csrc"), os.path.join(ROOT, "tests", "owners_host.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert built.returncode == 0, built.stderr[-3000:]
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=60)      # (run directly, never loaded into Python)
    print(ran.stdout)
    assert ran.returncode == 0, (ran.stdout + ran.stderr)[-3000:]
    assert ran.stdout.startswith("owners ok")
