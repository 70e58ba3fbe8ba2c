"""gk_lcp / Kmers.lcp, kmer_spectrum, min_unique_lengths, multiplicity_track: the parts that need no
GPU -- the exported symbols and their prototypes, the GKM_LCP_PATH knob, the null-context and Python
argument checks (made before any device call), and the two comparisons of
genome-kmers_amd/csrc/gkm_lcp_host.h under ``-fsanitize=address,undefined`` in a stand-alone driver
(tests/sanitize/lcp_driver.cpp).  Nothing is loaded into Python under a sanitizer."""

import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from genome_kmers import _native
from genome_kmers import kmers as gk

LCP_SYMBOLS = ("gk_lcp", "gk_copy_lcp", "gk_device_lcp", "gk_lcp_spectrum", "gk_position_track", "gk_device_track")


def test_lcp_is_exported():
    lib = _native.load_library()
    for name in LCP_SYMBOLS:
        assert name in _native.EXPORTED and name in _native._SIGS
        assert hasattr(lib, name)
    header = (ROOT / "include" / "gkm.h").read_text()
    for proto in ("int gk_lcp(gk_ctx *ctx, uint32_t max_len, uint64_t *n);",
                  "int gk_copy_lcp(gk_ctx *ctx, uint64_t offset, uint32_t *dst, uint64_t count);",
                  "int gk_device_lcp(gk_ctx *ctx, void **lcp, uint64_t *n);",
                  "int gk_lcp_spectrum(gk_ctx *ctx, uint32_t max_len, uint64_t *distinct, uint64_t *unique);",
                  "int gk_position_track(gk_ctx *ctx, int kind, uint32_t len, uint32_t *dst, uint64_t sba_len);",
                  "int gk_device_track(gk_ctx *ctx, void **track, uint64_t *sba_len);",
                  "#define GK_NEVER_UNIQUE 0xFFFFFFFFu", "#define GK_TRACK_MIN_UNIQUE 1",
                  "#define GK_TRACK_MULTIPLICITY 2"):
        assert proto in header, proto
    assert (_native.NEVER_UNIQUE, _native.TRACK_MIN_UNIQUE, _native.TRACK_MULTIPLICITY) == (0xFFFFFFFF, 1, 2)
    assert gk.NEVER_UNIQUE == 0xFFFFFFFF
    for method in ("lcp", "device_lcp", "lcp_spectrum", "position_track", "device_track"):
        assert callable(getattr(_native.Engine, method))
    for method in ("lcp", "kmer_spectrum", "min_unique_lengths", "multiplicity_track"):
        assert callable(getattr(gk.Kmers, method))


def test_tile_constants_the_gpu_tests_mirror():
    """tests/test_gpu_lcp.py places its edges by these values of gkm_lcp_host.h."""
    text = (ROOT / "genome-kmers_amd" / "csrc" / "gkm_lcp_host.h").read_text()
    values = {name: int(v) for name, v in re.findall(r"constexpr (?:uint32_t|int) (k\w+) = (\d+);", text)}
    assert (values["kThreads"], values["kItems"], values["kLdsBins"]) == (256, 4, 1024)
    assert "#define GKM_LCP_PEEL_ROUNDS 1\n" in text
    assert "constexpr uint32_t kTile = kThreads * kItems;" in text
    assert "constexpr uint32_t kMaxCap = 1u << 24;" in text


def test_lcp_knob_is_in_the_table():
    lib = _native.load_library()
    for value in ("bytes", "keys"):
        _native.options["GKM_LCP_PATH"] = value
        assert _native.options.get("GKM_LCP_PATH") == value
        del _native.options["GKM_LCP_PATH"]
        assert "GKM_LCP_PATH" not in _native.options
    for name in (b"GKM_LCP_PATHS", b"GKM_LCP", b"gkm_lcp_path"):
        assert lib.gk_set_option(name, b"bytes") == _native.GK_E_ARG
    # not an operational knob: the environment does not set it (gk_set_option only)
    text = (ROOT / "genome-kmers_amd" / "csrc" / "gkm_capi.hip").read_text()
    assert '{"GKM_LCP_PATH", false}' in text


def test_null_contexts():
    lib = _native.load_library()
    assert lib.gk_lcp(None, 31, None) == _native.GK_E_ARG
    assert lib.gk_copy_lcp(None, 0, None, 0) == _native.GK_E_ARG
    assert lib.gk_device_lcp(None, None, None) == _native.GK_E_ARG
    assert lib.gk_lcp_spectrum(None, 31, None, None) == _native.GK_E_ARG
    assert lib.gk_position_track(None, _native.TRACK_MIN_UNIQUE, 31, None, 0) == _native.GK_E_ARG
    assert lib.gk_position_track(None, _native.TRACK_MULTIPLICITY, 0, None, 0) == _native.GK_E_ARG
    assert lib.gk_device_track(None, None, None) == _native.GK_E_ARG


def host_kmers(kmin, kmax, is_sorted=True):
    """A Kmers with no sequence collection and no engine: the state the argument checks read."""
    km = gk.Kmers(None, min_kmer_len=kmin, max_kmer_len=kmax)
    km._is_sorted = is_sorted
    return km


@pytest.mark.parametrize("method,name", [("lcp", "max_len"), ("kmer_spectrum", "max_len"),
                                         ("min_unique_lengths", "max_len"), ("multiplicity_track", "kmer_len")])
def test_python_argument_checks_need_no_device(method, name):
    with pytest.raises(AssertionError, match=f"must be sorted when calling {method}"):
        getattr(host_kmers(21, 21, is_sorted=False), method)()
    with pytest.raises(AssertionError, match=f"must be sorted when calling {method}"):
        getattr(host_kmers(21, 21, is_sorted=False), method)(5)
    call = getattr(host_kmers(8, 21), method)
    for bad in (0, -3):
        with pytest.raises(ValueError, match=rf"{name} \({bad}\) must be >= 1"):
            call(bad)
    for bad in (2.0, "7", True, [3]):
        with pytest.raises(ValueError, match=f"{name} must be an int >= 1"):
            call(bad)
    with pytest.raises(ValueError, match=rf"{name} \(22\) is greater than max_kmer_len \(21\)"):
        call(22)
    with pytest.raises(ValueError, match=rf"{name} \(22\) is greater than max_kmer_len \(21\)"):
        call(np.int64(22))
    other = host_kmers(21, 21)
    other.kmer_source_strand = "both"
    with pytest.raises(ValueError, match="kmer_source_strand 'forward'"):
        getattr(other, method)(5)
    if name == "max_len":  # the suffix order has no length of its own
        with pytest.raises(ValueError, match=f"{method} needs max_len when max_kmer_len is None"):
            getattr(host_kmers(5, None), method)()


SAN_FLAGS = ["-std=c++17", "-g", "-O1", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=all"]


def test_comparisons_under_asan_ubsan(tmp_path):
    # the only thing that may skip: no g++, or a g++ without the sanitizer runtime, shown by a
    # one-line program that does not build with the same flags
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if shutil.which("g++") is None or subprocess.run(
            ["g++", *SAN_FLAGS, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("no g++ with the address / undefined-behaviour sanitizer runtime")
    exe = tmp_path / "lcp_asan"
    r = subprocess.run(["g++", *SAN_FLAGS, "-I", str(ROOT / "genome-kmers_amd" / "csrc"),
                        str(ROOT / "tests" / "sanitize" / "lcp_driver.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    bad = ("AddressSanitizer", "runtime error:", "LeakSanitizer")
    assert r.returncode == 0 and not any(b in r.stderr for b in bad), (r.returncode, r.stderr[-3000:])
    assert r.stdout.strip() == "ok"
