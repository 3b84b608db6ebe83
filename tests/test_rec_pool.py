"""The shard scheduler and its job pool (csrc/rec_pool.hpp) alone, on the CPU: tools/rec_pool_check.cpp runs the
scheduling loop with fake leaves, aggregations and batches that only record which jobs they carried -- n in
{1, 2, 3, 5, 8, 13, 32} x 1, 2, 4 threads x both tree shapes, with a failing leaf and a failing rider -- as a stand-alone
program under the thread sanitizer and, built a second time, under the address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "rec_pool_check.cpp")


@pytest.mark.parametrize("name,flags", [("thread", ["-fsanitize=thread"]),
                                        ("address_undefined", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])])
def test_scheduler_with_fake_provers_under_sanitizers(tmp_path, name, flags):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / ("rec_pool_check_" + name))
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-pthread", "-Wall", "-Wextra", "-Werror", *flags, SRC, "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, TSAN_OPTIONS="halt_on_error=1", ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    assert "WARNING: ThreadSanitizer" not in r.stderr and "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
    last = r.stdout.strip().splitlines()[-1]
    assert last.endswith(" cases, 0 failed") and int(last.split()[0]) >= 7 * 3 * 2, last
