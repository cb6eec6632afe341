"""Host-side native tests of the grouped GEMM: its tile map (tests/native/
test_gemm_grouped_map.cpp) and what ``gemm_launch`` decides for a grouped launch against stub
entries (tests/native/test_gemm_grouped_dispatch.cpp). Both are stand-alone host programs compiled
with AddressSanitizer + UndefinedBehaviorSanitizer; the assertions are in the programs."""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")

needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC) and shutil.which("hipcc") is None,
                                 reason="hipcc not installed")


def _build_and_run(tmp_path, source, ok_line):
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    exe = str(tmp_path / os.path.splitext(source)[0])
    cmd = [hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", f"-I{os.path.join(ROOT, 'csrc')}",
           os.path.join(ROOT, "tests", "native", source), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    # verify_asan_link_order=0: the process environment may preload other libraries; the
    # sanitizer runtime is linked into the test binary itself
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert ok_line in r.stdout
    assert " 0 checks failed" in r.stdout
    return r.stdout


@needs_hipcc
def test_gemm_grouped_map_host_asan_ubsan(tmp_path):
    """Every workgroup index of the grid bound, for BM in {128, 256}, E in 1..9 and a few thousand
    offset vectors (empty, single-row, multiples of BM, non-monotone, beyond T): each tile of the
    clamped offsets exactly once, "no tile" for the rest, no row outside [0, T)."""
    out = _build_and_run(tmp_path, "test_gemm_grouped_map.cpp", "grouped map ok")
    assert int(out.split(" vectors")[0].split()[-1]) >= 3000


@needs_hipcc
def test_gemm_grouped_dispatch_host_asan_ubsan(tmp_path):
    """Each accepted grouped form reaches ``launch_grouped`` with its arguments, an offered tile
    and the grid bound; each refusal (flags, tables, grouped rows, K-split, all-gather, unit-scale
    fp8, f32 / f64, mode generic, ping-pong / interleaved / 256x256 codes, ngroups out of range,
    overlapping weights, misaligned scale strides, ...) launches nothing."""
    _build_and_run(tmp_path, "test_gemm_grouped_dispatch.cpp", "grouped dispatch ok")
