"""CPU: the K1 hash and register probe (dd_k1.h: mul64_c32, mul64_c32_fold, wang64_fast, probe, RegsLds::at) as plain host code --
tests/native/k1_hash.hip, a stand-alone program built from the host side of the source alone: the gfx950 arrangement of
Wang's mix (the multiply by 265 with its high product folded into the mad's addend) against dd::wang64 on edge word pairs, on the keys that bring those pairs to the multiply by 265 and on more than
a million random values; the probe against the register's LDS address, the 32 bits behind the index and the leading-zero count
for every log2m 4 .. 16 and every slot within 160 KiB.  Built under AddressSanitizer + UBSan (host code only) where that build
links; where it does not, built plain.  Either way the program is run and must pass: a build that fails both ways fails the
test."""
import os
import re
import subprocess

from dandd_amd.build import hipcc

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "dandd_amd", "csrc")
SANITIZE = ["-Xarch_host", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"]


def test_hash_and_probe_equal_their_definitions(tmp_path):
    exe = str(tmp_path / "k1_hash")
    base = [hipcc(), "--offload-host-only", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unused-function", "-I" + CSRC,
            os.path.join(HERE, "native", "k1_hash.hip"), "-o", exe]
    b = subprocess.run(base + SANITIZE, capture_output=True, text=True, timeout=600)
    if b.returncode != 0:
        print("sanitizer build failed, building plain:\n" + b.stderr[-1500:])
        b = subprocess.run(base, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "k1_hash: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    m = re.search(r"k1_hash: ok \((\d+) comparisons\)", r.stdout)
    # 36 + 36 + 1.3 M hashes in both forms, and 67 hashes x 20 470 slots x 5 probe comparisons
    assert m and int(m.group(1)) > 2_600_000 + 6_000_000, r.stdout[-500:]
