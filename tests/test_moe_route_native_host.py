"""Host-side native test of the MoE routing sort's index arithmetic (csrc/moe/moe_route_map.h,
tests/native/test_moe_route_map.cpp): a stand-alone host program compiled with AddressSanitizer +
UndefinedBehaviorSanitizer; the assertions are in the program."""

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
def test_moe_route_map_host_asan_ubsan(tmp_path):
    """Count / scan / place replayed on the host through the header's index functions for a few
    thousand (S * k, E, ids) vectors (chunk multiples +- 1, one expert taking everything, every
    id invalid, ids far outside int32): the result is the stable sort by expert without the
    dropped slots, every slot is taken once, and no index leaves its table."""
    out = _build_and_run(tmp_path, "test_moe_route_map.cpp", "route map ok")
    assert int(out.split(" vectors")[0].split()[-1]) >= 3000
