"""Groups of transactions (bp_tune_txn_group) on the CPU: tools/txn_group_check.cpp runs the shard scheduler's group rule
(csrc/rec_pool.hpp) and the group lease's bookkeeping (csrc/worker_table.hpp, the real code behind a fake worker table)
with fake provers -- n = 1..40 leaves x 1..8 threads x groups of 1..3, leases that grant fewer than asked, a failing
member, an abort in mid-run; group leases beside single leases on 1..9 workers in 1..3 slabs -- as a stand-alone program
under the thread sanitizer and, built a second time, under the address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "txn_group_check.cpp")


@pytest.mark.parametrize("name,flags", [("thread", ["-fsanitize=thread"]),
                                        ("address_undefined", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])])
def test_groups_with_fake_provers_under_sanitizers(tmp_path, name, flags):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / ("txn_group_check_" + name))
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-pthread", "-Wall", "-Wextra", "-Werror", *flags, SRC, "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, TSAN_OPTIONS="halt_on_error=1", ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    assert "WARNING: ThreadSanitizer" not in r.stderr and "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
    last = r.stdout.strip().splitlines()[-1]
    # 40 sizes x 8 thread counts x (2 + 3 + 3) scheduler cases, and the lease cases
    assert last.endswith(" cases, 0 failed") and int(last.split()[0]) >= 40 * 8 * 8, last
