"""The owners of the host layer (f_renderer_amd/csrc/frr_own.h: DevBuf, Event) without a GPU and without the HIP runtime:
tests/own_host.cpp defines the four HIP calls they make over malloc, with a set of live blocks that aborts on a double or
foreign free, and is built with the address and undefined-behaviour sanitizers.  It passes only if the program exits 0 and
no sanitizer has reported anything."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def test_owners_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "own_host")
    subprocess.check_call([gxx, "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"),
                           "-I" + os.path.join(ROOT, "f_renderer_amd", "csrc"), "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-o", exe, os.path.join(ROOT, "tests", "own_host.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("own_host: ok"), r.stdout
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
