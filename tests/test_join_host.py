"""gk_join / Kmers.compare, the parts that need no GPU: the exported symbols and their prototypes, the
GKM_JOIN_PATH knob, the Python argument checks (made before any device call), and the index
arithmetic of the key path (genome-kmers_amd/csrc/gkm_join_host.h: the merge-path diagonal search
and the tile kernels' bounds) under ``-fsanitize=address,undefined`` in a stand-alone driver
(tests/sanitize/join_driver.cpp).  Nothing is loaded into Python under a sanitizer."""

import os
import shutil
import subprocess

import pytest

from conftest import ROOT
from genome_kmers import _native
from genome_kmers import kmers as gk

JOIN_SYMBOLS = ("gk_join", "gk_copy_join", "gk_device_join", "gk_join_mask")


def test_join_is_exported():
    lib = _native.load_library()
    for name in JOIN_SYMBOLS:
        assert name in _native.EXPORTED and name in _native._SIGS
        assert hasattr(lib, name)
    header = (ROOT / "include" / "gkm.h").read_text()
    for proto in ("int gk_join(gk_ctx *a, gk_ctx *b, uint32_t flags, gk_join_stats *stats);",
                  "int gk_copy_join(gk_ctx *a, uint64_t *b_first, uint32_t *b_count, uint64_t n);",
                  "int gk_device_join(gk_ctx *a, void **b_first, void **b_count, uint64_t *n);",
                  "int gk_join_mask(gk_ctx *a, int keep);",
                  "#define GK_JOIN_KEEP_ABSENT 1", "#define GK_JOIN_KEEP_PRESENT 2"):
        assert proto in header, proto
    assert (_native.JOIN_KEEP_ABSENT, _native.JOIN_KEEP_PRESENT) == (1, 2)
    # the stats record: six uint64 in the header's order
    assert [n for n, _ in _native.GkJoinStats._fields_] == ["n_distinct_a", "n_distinct_b", "n_shared",
                                                            "occ_a_shared", "occ_b_shared", "occ_min"]
    import ctypes
    assert ctypes.sizeof(_native.GkJoinStats) == 48
    for method in ("join", "join_result", "join_mask"):
        assert callable(getattr(_native.Engine, method))


def test_join_knob_is_in_the_table():
    lib = _native.load_library()
    for value in ("bytes", "keys"):
        _native.options["GKM_JOIN_PATH"] = value
        assert _native.options.get("GKM_JOIN_PATH") == value
        del _native.options["GKM_JOIN_PATH"]
        assert "GKM_JOIN_PATH" not in _native.options
    for name in (b"GKM_JOIN_PATHS", b"GKM_JOIN", b"gkm_join_path"):
        assert lib.gk_set_option(name, b"bytes") == _native.GK_E_ARG
    # not an operational knob: the environment does not set it (gk_set_option only)
    text = (ROOT / "genome-kmers_amd" / "csrc" / "gkm_capi.hip").read_text()
    assert '{"GKM_JOIN_PATH", false}' in text


def test_null_contexts():
    lib = _native.load_library()
    assert lib.gk_join(None, None, 0, None) == _native.GK_E_ARG
    assert lib.gk_copy_join(None, None, None, 0) == _native.GK_E_ARG
    assert lib.gk_device_join(None, None, None, None) == _native.GK_E_ARG
    assert lib.gk_join_mask(None, 1) == _native.GK_E_ARG


def host_kmers(kmin, kmax, is_sorted=True, canonical=False):
    """A Kmers with no sequence collection and no engine: the state the argument checks read."""
    km = gk.Kmers(None, min_kmer_len=kmin, max_kmer_len=kmax)
    km._is_sorted = is_sorted
    km._canonical = canonical
    return km


@pytest.mark.parametrize("method", ["count_in", "compare", "absent_from", "present_in"])
def test_python_argument_checks_need_no_device(method):
    a = host_kmers(21, 21)
    call = getattr(a, method)
    with pytest.raises(ValueError, match="two Kmers objects.*other: str"):
        call("ACGT")
    with pytest.raises(AssertionError, match=f"must be sorted when calling {method}.*self sorted: True.*other sorted: False"):
        call(host_kmers(21, 21, is_sorted=False))
    with pytest.raises(AssertionError, match="self sorted: False"):
        getattr(host_kmers(21, 21, is_sorted=False), method)(a)
    other = host_kmers(21, 21)
    other.kmer_source_strand = "both"
    with pytest.raises(ValueError, match="'forward' on both sides.*self: 'forward', other: 'both'"):
        call(other)
    with pytest.raises(ValueError, match=r"one fixed max_kmer_len on both sides \(self: 21, other: 31\)"):
        call(host_kmers(31, 31))
    with pytest.raises(ValueError, match=r"one fixed max_kmer_len on both sides \(self: None, other: None\)"):
        getattr(host_kmers(5, None), method)(host_kmers(5, None))
    with pytest.raises(ValueError, match=r"min_kmer_len == max_kmer_len.*other: min_kmer_len = 8, max_kmer_len = 21"):
        call(host_kmers(8, 21))
    with pytest.raises(ValueError, match=r"min_kmer_len == max_kmer_len.*self: min_kmer_len = 8, max_kmer_len = 21"):
        getattr(host_kmers(8, 21), method)(a)
    with pytest.raises(ValueError, match="canonical or not.*self canonical: False, other canonical: True"):
        call(host_kmers(21, 21, canonical=True))


def test_join_filter_refuses_every_other_use():
    a, b = host_kmers(21, 21), host_kmers(21, 21)
    for filt in (a.absent_from(b), a.present_in(b)):
        assert isinstance(filt, gk._JoinFilter) and filt.owner is a and filt.other is b
        with pytest.raises(TypeError, match="cannot be called as"):
            filt(None, "forward", 0)
        # the array-level module functions know no Kmers
        with pytest.raises(ValueError, match="array-level functions"):
            gk._device_filter(None, filt, None, "forward", lambda: [])
        with pytest.raises(ValueError, match="another Kmers object"):
            gk._device_filter(None, filt, None, "forward", lambda: [], owner=b, kmer_len=21)
        with pytest.raises(ValueError, match=r"max_kmer_len \(21\) only \(kmer_len = 20\)"):
            gk._device_filter(None, filt, None, "forward", lambda: [], owner=a, kmer_len=20)
    assert (a.absent_from(b).keep, a.present_in(b).keep) == (_native.JOIN_KEEP_ABSENT, _native.JOIN_KEEP_PRESENT)


SAN_FLAGS = ["-std=c++17", "-g", "-O1", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=all"]


def test_diagonal_search_under_asan_ubsan(tmp_path):
    # the only thing that may skip: no g++, or a g++ without the sanitizer runtime, shown by a
    # one-line program that does not build with the same flags
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if shutil.which("g++") is None or subprocess.run(
            ["g++", *SAN_FLAGS, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("no g++ with the address / undefined-behaviour sanitizer runtime")
    exe = tmp_path / "join_asan"
    r = subprocess.run(["g++", *SAN_FLAGS, "-I", str(ROOT / "genome-kmers_amd" / "csrc"),
                        str(ROOT / "tests" / "sanitize" / "join_driver.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    bad = ("AddressSanitizer", "runtime error:", "LeakSanitizer")
    assert r.returncode == 0 and not any(b in r.stderr for b in bad), (r.returncode, r.stderr[-3000:])
    assert r.stdout.strip() == "ok"
