"""the CPU side under -fsanitize=address,undefined.

The plain-C/C++ host code of the product (csrc/host_groups.c: incremental grouping walk with
caches kept across calls; csrc/host_rng.c: numpy's Mersenne-Twister state stepped in place;
csrc/host_constrainer.cpp: the native constrainer) and the oracle's C restatement
(oracle/mdns_oracle.c) are rebuilt with AddressSanitizer + UndefinedBehaviorSanitizer into a
temporary directory and the tests that exercise them are replayed in a child interpreter that
loads THOSE builds (MDNS_HOST_LIB / MDNS_ORACLE_LIB): any report fails the test.  (GPU
AddressSanitizer is not available on the pool; the kernels are checked against the oracle.)"""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "massivedatans_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]


def _gcc_file(name):
    out = subprocess.run(["gcc", "-print-file-name=" + name], capture_output=True, text=True).stdout.strip()
    return out if os.path.sep in out and os.path.exists(out) else None


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    asan = _gcc_file("libasan.so")
    if asan is None:
        pytest.skip("no libasan in this toolchain")
    out = tmp_path_factory.mktemp("san")
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC]
    objs = []
    for src, cc, std in (("host_groups.c", "gcc", "-std=c99"), ("host_rng.c", "gcc", "-std=c99"),
                         ("host_constrainer.cpp", "g++", "-std=c++17"), ("host_sampler.cpp", "g++", "-std=c++17")):
        obj = str(out / (src + ".o"))
        subprocess.run([cc, std, "-fPIC", "-ffp-contract=off", "-Wall"] + SAN + inc + ["-c", os.path.join(CSRC, src), "-o", obj], check=True)
        objs.append(obj)
    host = str(out / "libmdns_host_san.so")
    subprocess.run(["g++", "-shared", "-fPIC"] + SAN + objs + ["-o", host, "-lm"], check=True)
    orc = str(out / "liboracle_san.so")
    subprocess.run(["gcc", "-std=c99", "-fPIC", "-ffp-contract=off"] + SAN +
                   [os.path.join(ROOT, "oracle", "mdns_oracle.c"), "-o", orc, "-shared", "-lm"], check=True)
    env = dict(os.environ, MDNS_HOST_LIB=host, MDNS_ORACLE_LIB=orc, LD_PRELOAD=asan,
               ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    return env


def _replay(env, selection):
    cmd = [sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", "-m", "not gpu"] + selection
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    text = out.stdout + out.stderr
    assert "AddressSanitizer" not in text and "runtime error:" not in text, text[-4000:]
    assert out.returncode == 0, text[-4000:]
    assert " passed" in text
    return text


def test_grouping_walk_and_bootstrap_draws_under_sanitizers(sanitized):
    _replay(sanitized, ["tests/test_sampler_units.py", "-k", "walk or bootstrap or superpoint or networkx"])


def test_oracle_restatement_under_sanitizers(sanitized):
    _replay(sanitized, ["tests/test_oracle.py"])


def test_native_constrainer_traces_under_sanitizers(sanitized):
    """The native constrainer end to end (region builds, all proposal kinds, metric refits, the
    chunked accept loop) on the two reference traces that reach every branch quickly; the selection takes the
    modes "native" and "native-chain", so the hand-over of a chained first batch runs here too, and the draws
    that its cross-checks end with an error."""
    _replay(sanitized, ["tests/test_orchestration.py", "-k", "(native and (nothing4 or horns3 or horns12)) or cross_checks"])


def test_sampler_core_under_sanitizers(sanitized):
    """The sampler core (csrc/host_sampler.cpp: passes, grouping -- fresh and kept up to date --, constrainer
    cache, shelves) on reference traces in both grouping modes, and the grouping stress test."""
    env = dict(sanitized, MDNS_CORE_CHECK_GROUPS="1")
    _replay(env, ["tests/test_orchestration.py", "tests/test_core.py", "-k",
                  "test_fresh_and_incremental or (core and (nothing4 or horns3 or horns12))"])
