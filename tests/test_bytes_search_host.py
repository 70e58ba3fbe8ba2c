"""The byte path's comparison and range search, shared by gk_lookup, gk_join and gk_screen
(genome-kmers_amd/csrc/gkm_bytes_search.h), on the CPU under ``-fsanitize=address,undefined`` in a
stand-alone driver (tests/sanitize/bytes_search_driver.cpp): every source of the sought k-mer,
forward and canonical orders, k = 1 .. 64, against brute-force counts, over an sba that ends at its
last '$' with no pad."""

import os
import shutil
import subprocess

import pytest

from conftest import ROOT

SAN_FLAGS = ["-std=c++17", "-g", "-O1", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=all"]


def test_bytes_search_under_asan_ubsan(tmp_path):
    # the only thing that may skip: no g++, or a g++ without the sanitizer runtime, shown by a
    # one-line program that does not build with the same flags
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if shutil.which("g++") is None or subprocess.run(
            ["g++", *SAN_FLAGS, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("no g++ with the address / undefined-behaviour sanitizer runtime")
    exe = tmp_path / "bytes_search_asan"
    r = subprocess.run(["g++", *SAN_FLAGS, "-I", str(ROOT / "genome-kmers_amd" / "csrc"),
                        str(ROOT / "tests" / "sanitize" / "bytes_search_driver.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    bad = ("AddressSanitizer", "runtime error:", "LeakSanitizer")
    assert r.returncode == 0 and not any(b in r.stderr for b in bad), (r.returncode, r.stderr[-3000:])
    assert r.stdout.strip() == "ok"
