"""The host side of K1's saturation exit without a GPU: which ks of a call are checked against sketch(U_k)
(dd_plan.h: plan_saturate_last_k), the two knobs, |U_k|, and that the job tables do not depend on any of it --
tests/native/saturate_gate.cpp, a program of its own under AddressSanitizer + UBSan."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "dandd_amd", "csrc")


def test_saturation_gate_and_knobs(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ needed")
    exe = str(tmp_path / "saturate_gate")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__",
           "-I/opt/rocm/include", "-I" + CSRC, "-x", "c++", os.path.join(HERE, "native", "saturate_gate.cpp"),
           os.path.join(CSRC, "dd_plan.hip"), "-o", exe, "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if b.returncode != 0 and "cannot find" in b.stderr:
        pytest.skip("sanitizer runtime not installed: " + b.stderr[-300:])
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "saturate_gate: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
