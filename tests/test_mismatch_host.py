"""gk_lookup_mismatch / Kmers.find_near, the parts that need no GPU: the exported symbol, the two
knobs of gk_set_option, the null-context answer, and the host-only C++ (reverse complement, 2-bit and
4-bit query words, chunk arithmetic, the hit-record sort and split:
genome-kmers_amd/csrc/gkm_mismatch_host.h) under ``-fsanitize=address,undefined`` in a stand-alone
driver (tests/sanitize/mismatch_driver.cpp)."""

import os
import shutil
import subprocess

import pytest

from conftest import ROOT
from genome_kmers import _native


def test_mismatch_is_exported():
    lib = _native.load_library()
    assert "gk_lookup_mismatch" in _native.EXPORTED and "gk_lookup_mismatch" in _native._SIGS
    assert hasattr(lib, "gk_lookup_mismatch")
    assert _native.MISMATCH_BOTH_STRANDS == 1
    header = (ROOT / "include" / "gkm.h").read_text()
    assert "#define GK_MISMATCH_BOTH_STRANDS 1u" in header
    flat = " ".join(header.split())
    assert ("int gk_lookup_mismatch(gk_ctx *ctx, const uint8_t *queries, uint64_t m, uint32_t qlen, "
            "uint32_t max_mismatches, uint32_t flags, uint64_t *counts, uint32_t *hit_query, "
            "uint64_t *hit_kmer_num, uint8_t *hit_mismatches, uint8_t *hit_strand, uint64_t capacity, "
            "uint64_t *n_hits);") in flat
    for name in ("mismatch_counts", "mismatch_hits"):
        assert callable(getattr(_native.Engine, name))


def test_mismatch_knobs_are_in_the_table():
    lib = _native.load_library()
    for name, value in (("GKM_MISMATCH_PATH", "bytes"), ("GKM_MISMATCH_PATH", "keys"), ("GKM_MISMATCH_CHUNK", "7")):
        _native.options[name] = value
        assert _native.options.get(name) == value
        del _native.options[name]
        assert name not in _native.options
    for name in (b"GKM_MISMATCH_PATHS", b"GKM_MISMATCH", b"GKM_MISMATCH_CHUNKS", b"GKM_MISMATCHES_PATH",
                 b"gkm_mismatch_path"):
        assert lib.gk_set_option(name, b"1") == _native.GK_E_ARG
    # not operational knobs: the environment does not set them (gk_set_option only)
    text = (ROOT / "genome-kmers_amd" / "csrc" / "gkm_capi.hip").read_text()
    for name in ("GKM_MISMATCH_PATH", "GKM_MISMATCH_CHUNK"):
        assert f'{{"{name}", false}}' in text


def test_null_context():
    lib = _native.load_library()
    assert lib.gk_lookup_mismatch(None, None, 0, 5, 1, 0, None, None, None, None, None, 0, None) == _native.GK_E_ARG
    assert lib.gk_lookup_mismatch(None, None, 3, 5, 1, 0, None, None, None, None, None, 0, None) == _native.GK_E_ARG


SAN_FLAGS = ["-std=c++17", "-g", "-O1", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=all"]


def test_host_pieces_under_asan_ubsan(tmp_path):
    # the only thing that may skip: no g++, or a g++ without the sanitizer runtime, shown by a
    # one-line program that does not build with the same flags
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if shutil.which("g++") is None or subprocess.run(
            ["g++", *SAN_FLAGS, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("no g++ with the address / undefined-behaviour sanitizer runtime")
    exe = tmp_path / "mismatch_asan"
    r = subprocess.run(["g++", *SAN_FLAGS, "-I", str(ROOT / "genome-kmers_amd" / "csrc"),
                        str(ROOT / "tests" / "sanitize" / "mismatch_driver.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    bad = ("AddressSanitizer", "runtime error:", "LeakSanitizer")
    assert r.returncode == 0 and not any(b in r.stderr for b in bad), (r.returncode, r.stderr[-3000:])
    assert r.stdout.strip() == "ok"
