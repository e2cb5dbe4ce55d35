"""densecap_amd/csrc/scratch.h on the host alone: tests/scratch_host.cpp (its own main, counting stand-ins for the header's
runtime calls) is built by the host compiler with AddressSanitizer + UBSan and run as a child process.  It shows that the
call-scoped owner drains its stream once and frees once on every way out, that a failed allocation leaves nothing behind, that
the kept buffer only grows, drains before it replaces and counts its allocations, and that carve lists get 256-byte pieces."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scratch_owners_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "scratch_host")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "scratch_host.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, "build failed:\n" + b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, "a check failed, or a sanitizer report:\n" + r.stdout[-2000:] + r.stderr[-2000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-2000:]
    assert r.stdout.strip().splitlines()[-1] == "scratch_host ok"
