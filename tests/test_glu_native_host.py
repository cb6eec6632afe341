"""Host-side native test of the gated (GLU) GEMM's dispatch: ``gemm_launch`` against stub launch
entries (tests/native/test_gemm_glu_dispatch.cpp), compiled for the host only with
AddressSanitizer + UndefinedBehaviorSanitizer. The assertions are in the program."""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")


@pytest.mark.skipif(not os.path.exists(HIPCC) and shutil.which("hipcc") is None,
                    reason="hipcc not installed")
def test_gemm_glu_dispatch_host_asan_ubsan(tmp_path):
    """Each accepted gated form reaches its entry with ``glu = 1`` and an offered tile; one
    perturbation at a time (N off the modulus, a short ldc, a K-split, grouped rows, flags, a
    table, unit-scale fp8, f32, a ping-pong tile, mode generic, a short scale pitch, ...) is
    refused with no launch."""
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    exe = str(tmp_path / "gemm_glu_dispatch")
    cmd = [hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", f"-I{os.path.join(ROOT, 'csrc')}",
           os.path.join(ROOT, "tests", "native", "test_gemm_glu_dispatch.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    # verify_asan_link_order=0: the process environment may preload other libraries; the
    # sanitizer runtime is linked into the test binary itself
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "glu dispatch ok" in r.stdout
    assert " 0 checks failed" in r.stdout
