"""The argument ring's bookkeeping (csrc/arg_ring.hpp: where the batched kernels' argument blocks live between a launch
and its end) on the CPU: tools/arg_ring_check.cpp drives the header with a fake stream -- alignment; puts of 1, 8, 9 and
24 blocks of the largest block type; the full case, which asks for one wait and never lands on a live block; rewind
after a wait; blocks larger than the ring, which are refused -- as a stand-alone program, built plain and, a second
time, under the address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "arg_ring_check.cpp")


@pytest.mark.parametrize("name,flags", [("plain", ["-O2"]),
                                        ("address_undefined", ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])])
def test_ring_bookkeeping_with_a_fake_stream(tmp_path, name, flags):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / ("arg_ring_check_" + name))
    b = subprocess.run([cxx, "-std=c++17", "-g", "-Wall", "-Wextra", "-Werror", *flags, SRC, "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
    last = r.stdout.strip().splitlines()[-1]
    assert last.endswith(" cases, 0 failed") and int(last.split()[0]) >= 10000, last
