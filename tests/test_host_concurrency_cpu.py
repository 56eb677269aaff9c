"""The host logic between the HIP calls of the C-ABI, on the CPU (no GPU): opencorr_amd/csrc/host/single_combiner.h (the
combining front end of compute(POI*)) and opencorr_amd/csrc/host/chunk_pipeline.h (chunk schedule and feeder / copy-out
hand-off of the host-queue pipeline).  Both headers need nothing but the standard library; tests/cpp/single_combiner_stress.cpp
and tests/cpp/chunk_pipeline_check.cpp are stand-alone programs, built here with plain g++ -- once as they are and once with
-fsanitize=thread.

What the barrier modes are for: a leader that publishes a request's state and then reads the sleeper count, against an owner
that registers as a sleeper and then re-reads its state, needs a seq_cst fence on either side.  With release / acquire alone
the owner of a round's LAST batch can sleep with nobody left to wake it; the stress program's barrier rounds hung in 7 runs of 7
(8 threads; after 5 663 - 161 639 rounds in the four runs that recorded it) when built against a copy of the header without the
two fences.  A hang is a
failure by timeout."""
import os
import platform
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (-Wno-tsan: GCC warns that the sanitizer does not model atomic_thread_fence; every hand-over of data in these headers goes
# through a mutex or a release / acquire pair, the fences only order the two flag reads)
TSAN = ("-O1", "-g", "-fsanitize=thread", "-Wno-tsan")
# the barrier modes at the round count at which the unfenced protocol hung every time; the fenced one takes ~10 s
ROUNDS = 300000
THREADS = min(8, len(os.sched_getaffinity(0)))


def _build(out_dir, name, flags):
    exe = str(out_dir / (name + ("_tsan" if flags is TSAN else "")))
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pthread", *flags, os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", exe],
                   check=True, timeout=600)
    return exe


@pytest.fixture(scope="module")
def stress(tmp_path_factory):
    d = tmp_path_factory.mktemp("single_combiner")
    return {"plain": _build(d, "single_combiner_stress", ("-O2",)), "tsan": _build(d, "single_combiner_stress", TSAN)}


def _sanitized(cmd, timeout):
    """Runs a program built with the thread sanitizer.  Its fixed shadow-memory layout does not survive the address-space
    randomisation of kernels with 32 random mmap bits (GCC 11's runtime: "FATAL: ThreadSanitizer: unexpected memory mapping"),
    so the program -- this one process, nothing else -- runs with randomisation off where setarch can do that."""
    fixed = ["setarch", platform.machine(), "-R"]
    if not shutil.which("setarch") or subprocess.run(fixed + ["true"], capture_output=True).returncode != 0:
        fixed = []
    out = subprocess.run(fixed + cmd, capture_output=True, text=True, timeout=timeout)
    print(out.stdout, out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ThreadSanitizer" not in out.stderr
    return out.stdout


def _run(exe, mode, threads, rounds, timeout):
    out = subprocess.run([exe, mode, str(threads), str(rounds)], capture_output=True, text=True, timeout=timeout)
    print(out.stdout, out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr


@pytest.mark.parametrize("mode", ["barrier", "promote"])
def test_no_wakeup_is_lost_after_a_last_batch(stress, mode):
    _run(stress["plain"], mode, THREADS, ROUNDS, timeout=60)


def test_free_running_callers_are_all_served(stress):
    _run(stress["plain"], "free", THREADS, ROUNDS, timeout=60)


@pytest.mark.parametrize("mode,threads,rounds", [("free", 8, 50000), ("barrier", 8, 50000), ("promote", 8, 50000), ("promote", 64, 2000)])
def test_combiner_is_clean_under_thread_sanitizer(stress, mode, threads, rounds):
    _sanitized([stress["tsan"], mode, str(threads), str(rounds)], timeout=120)


def test_chunk_schedule_and_handoff(tmp_path):
    """The schedule pinned to the values of the expressions as they stood inline in capi_host.hip, and the hand-off between one
    feeder and one consumer thread, under the thread sanitizer."""
    exe = _build(tmp_path, "chunk_pipeline_check", TSAN)
    rows = [ln for ln in _sanitized([exe], timeout=120).splitlines() if ln.strip()]
    assert len(rows) == 12 and all(ln.endswith(" ok") for ln in rows)
