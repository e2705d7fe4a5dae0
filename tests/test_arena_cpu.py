"""The workspace carver (csrc/arena.h) under AddressSanitizer and UBSan on the host: tests/arena_layout.cpp carves every driver's
layout over a malloc of exactly the measured size, compares every offset and total with the formulas the drivers used before the
carver, and writes every element of every block.  A stand-alone program run as a child process; nothing is preloaded."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host_cxx():
    for name in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        path = shutil.which(name)
        if path:
            return path
    raise AssertionError("no host C++ compiler for the carver's layout program")


def test_every_driver_layout_matches_the_old_formulas_and_stays_inside_its_allocation(tmp_path):
    cxx, exe = _host_cxx(), tmp_path / "arena_layout"
    # the sanitizer runtimes linked into the program itself (clang's default; GCC links them dynamically unless told)
    gcc = "clang" not in subprocess.check_output([cxx, "--version"], text=True)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
                          + (["-static-libasan", "-static-libubsan"] if gcc else [])
                          + ["-I", os.path.join(ROOT, "surface-sampling_amd", "csrc"), os.path.join(ROOT, "tests", "arena_layout.cpp"), "-o", str(exe)])
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().endswith("ok: 0 failure(s)"), run.stdout
