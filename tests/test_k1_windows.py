"""CPU: the slice arithmetic of the K1 windows (dd_k1.h: funnel32, SegWords, Windows<...>::slice) as plain host code --
tests/native/k1_windows.hip, a stand-alone program built from the host side of the source alone: every window form, every
word and token position of a segment and every k of its class against token-by-token pushes.  Built under AddressSanitizer +
UBSan (host code only) where that build links; where it does not, built plain.  Either way the program is run and must pass:
a build that fails both ways fails the test."""
import os
import subprocess

from dandd_amd.build import hipcc

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "dandd_amd", "csrc")
SANITIZE = ["-Xarch_host", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"]


def test_slices_equal_pushes(tmp_path):
    exe = str(tmp_path / "k1_windows")
    base = [hipcc(), "--offload-host-only", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unused-function", "-I" + CSRC,
            os.path.join(HERE, "native", "k1_windows.hip"), "-o", exe]
    b = subprocess.run(base + SANITIZE, capture_output=True, text=True, timeout=600)
    if b.returncode != 0:
        print("sanitizer build failed, building plain:\n" + b.stderr[-1500:])
        b = subprocess.run(base, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "k1_windows: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
