"""CPU sanitizer leg for the record index of dd_io.h (dd_fasta_index): tests/native/sanitize_index.cpp, a stand-alone program,
under AddressSanitizer + UBSan -- known tables, every truncation of odd buffers in heap blocks of exactly their size, and
the loaders on plain and gzip files."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "dandd_amd", "csrc")


def test_record_index_under_asan_ubsan(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ needed")
    exe = str(tmp_path / "sanitize_index")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__",
           "-I/opt/rocm/include", "-I" + CSRC, "-x", "c++", os.path.join(HERE, "native", "sanitize_index.cpp"),
           "-o", exe, "-L/opt/rocm/lib", "-lamdhip64", "-lz", "-ldl", "-lpthread", "-Wl,-rpath,/opt/rocm/lib"]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if b.returncode != 0 and "cannot find" in b.stderr:
        pytest.skip("sanitizer runtime not installed: " + b.stderr[-300:])
    assert b.returncode == 0, b.stderr[-3000:]
    work = tmp_path / "files"
    work.mkdir()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    for extra in ({}, {"DD_NO_LIBDEFLATE": "1"}):
        r = subprocess.run([exe, str(work)], env=dict(env, **extra), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "sanitize_index: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
