"""The interval search over rank blocks (nolzss_amd/csrc/rank_blocks.hpp) on the CPU: tests/host/rank_blocks_test.cpp
is compiled as a stand-alone program -- with the address and undefined-behaviour sanitizers where the compiler has
them -- and compares lo / hi / min SA with the entry-by-entry scans on random arrays.  No GPU, nothing loaded into
Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_block_search_against_plain_scans(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "rank_blocks_test"
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-I", os.path.join(ROOT, "nolzss_amd", "csrc"),
            os.path.join(ROOT, "tests", "host", "rank_blocks_test.cpp"), "-o", str(exe)]
    # (the sanitizer runtimes linked statically: the program then runs the same whatever else the process preloads)
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"],
                       capture_output=True, text=True)
    if r.returncode != 0:  # (a compiler without these runtimes)
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout[-2000:] + r.stderr[-4000:]
