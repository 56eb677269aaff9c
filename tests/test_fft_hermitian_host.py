"""The real-output inverse 32-point transform of opencorr_amd/csrc/fft_device.h (ifft32_hermitian: the last pass of the 32 x 32
FFTCC2D kernel) on the HOST (no GPU): tests/cpp/fft_hermitian_host_check.hip feeds it random Hermitian lines and compares the 32
real outputs with a double-precision DFT, under the relative-error bar of tests/cpp/fft_host_check.hip."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_real_output_inverse_fft32_matches_a_double_precision_dft(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    exe = str(tmp_path / "fft_hermitian_host_check")
    src = os.path.join(ROOT, "tests", "cpp", "fft_hermitian_host_check.hip")
    # -ffp-contract=off like the library (the butterflies opt back in with their own pragma)
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-ffp-contract=off", src, "-o", exe], check=True,
                   cwd=str(tmp_path), timeout=900)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    rows = [ln.split() for ln in out.stdout.splitlines() if ln.strip()]
    assert out.returncode == 0, out.stdout
    assert len(rows) == 16 and all(r[0] == "32" and r[2] == "ok" for r in rows)
    assert max(float(r[1]) for r in rows) < 5e-7
