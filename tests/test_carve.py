"""mv::Carve, the one description of every device scratch layout (maveric-slam_amd/csrc/hip/mv_carve.hpp),
on the CPU: tests/c/carve_check.cpp built with g++ under AddressSanitizer + UndefinedBehaviorSanitizer
and run.  The header is plain C++17, so the check needs neither HIP nor a device: a measuring pass and
a real pass give the same offsets and bytes(), arrays start on 256-B boundaries, do not overlap and end
at bytes(), a zero-count take is valid, and every byte of a 5-array layout with odd counts can be
written inside a block of exactly bytes() bytes."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANFLAGS = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def test_carve_under_asan_ubsan():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "carve_check")
        r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror",
                            "-I" + os.path.join(ROOT, "maveric-slam_amd", "csrc", "hip")] + SANFLAGS +
                           ["-o", exe, os.path.join(ROOT, "tests", "c", "carve_check.cpp")],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
        r = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
        assert r.returncode == 0 and "runtime error" not in r.stderr, r.stderr[-4000:]
        assert "carve_check ok" in r.stdout
