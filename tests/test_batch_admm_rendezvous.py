"""The two meetings of a batched solve (csrc/lrs_batch_rdv.h: one rendezvous for the ALM phase, a
second one for the ADMM phase) without a GPU: tests/c/batch_admm_rendezvous.cpp drives two
BatchRendezvous objects with stub launchers -- members that move from the first quorum to the
second at different times, members that never join the second, an error return out of the ADMM
phase, a failing ADMM round, and two scenarios that end only if a member in one phase never waits
for a member in the other.  The program checks that every call is served exactly once by its own
meeting; here it gets a time limit (it must end)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "batch_admm_rendezvous.cpp")


def _build(tmp_path, name, extra):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / name)
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-pthread", *extra, SRC, "-o", exe],
                       capture_output=True, text=True)
    return exe, r


def test_two_rendezvous_program(tmp_path):
    exe, r = _build(tmp_path, "batch_admm_rendezvous", [])
    assert r.returncode == 0, r.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == "ok"


def test_two_rendezvous_program_thread_sanitizer(tmp_path):
    """The same program under the host toolchain's thread sanitizer, where it has the runtime."""
    exe, r = _build(tmp_path, "batch_admm_rendezvous_tsan", ["-fsanitize=thread"])
    if r.returncode != 0:
        pytest.skip("the host toolchain has no thread sanitizer runtime")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    if out.returncode != 0 and "FATAL: ThreadSanitizer: unexpected memory mapping" in out.stderr and not out.stdout:
        # the runtime could not set up its shadow memory under this kernel's address-space
        # randomisation: it never reached main()
        pytest.skip("the thread sanitizer's runtime cannot start on this machine")
    assert out.returncode == 0, out.stderr[-4000:]
    assert "ThreadSanitizer" not in out.stderr
    assert out.stdout.strip() == "ok"
