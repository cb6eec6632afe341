"""Host-side native tests of the K-grouped GEMM: the padded K layout it shares with the grouped
transposing quantiser (tests/native/test_gemm_kgrouped_map.cpp) and what ``gemm_launch`` decides
for a K-grouped launch against stub entries (tests/native/test_gemm_kgrouped_dispatch.cpp). Both
are stand-alone host programs compiled with AddressSanitizer + UndefinedBehaviorSanitizer, built
and run as tests/test_gemm_grouped_native_host.py builds its two; the assertions are in the
programs."""

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
def test_gemm_kgrouped_map_host_asan_ubsan(tmp_path):
    """For MOD in {128, 256}, E in 1..9 and a few thousand offset vectors (empty, one row,
    multiples of MOD plus or minus 1, non-monotone, negative, beyond T): the groups' column ranges
    are disjoint, ascending multiples of MOD that cover their rows, ``k0_E`` stays within the
    capacity and attains it for some vector, nothing is read past ``o[E]``, and the quantiser's
    (tile -> group, rows, destination column) map agrees with the GEMM's range for every tile."""
    out = _build_and_run(tmp_path, "test_gemm_kgrouped_map.cpp", "kgrouped map ok")
    assert int(out.split(" vectors")[0].split()[-1]) >= 3000
    assert int(out.split(" attain the capacity")[0].split()[-1]) > 0


@needs_hipcc
def test_gemm_kgrouped_dispatch_host_asan_ubsan(tmp_path):
    """Each accepted K-grouped form reaches ``launch_kgrouped`` with its arguments, an offered tile
    and a grid that is one; each refusal (flags, tables, grouped rows, K-split, all-gather, tile
    codes, ngroups out of range, act, glu, a quantised output, unscaled or 16-bit operands, a
    column extent below the capacity, overlapping or misaligned group outputs, a grid past
    2^31 - 1, ...) launches nothing."""
    _build_and_run(tmp_path, "test_gemm_kgrouped_dispatch.cpp", "kgrouped dispatch ok")
