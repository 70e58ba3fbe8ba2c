"""gk_lookup / Kmers.find, the parts that need no GPU: query packing (_native.pack_queries), the
exported symbol, the lookup knobs of gk_set_option, and the host-only C++ (query validation,
canonical form, chunk arithmetic: genome-kmers_amd/csrc/gkm_lookup_host.h) under
``-fsanitize=address,undefined`` in a stand-alone driver (tests/sanitize/lookup_driver.cpp)."""

import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from genome_kmers import _native


def test_pack_queries_input_forms():
    one = _native.pack_queries("ACGTN")
    assert one.dtype == np.uint8 and one.shape == (1, 5) and one.flags.c_contiguous
    assert bytes(one[0]) == b"ACGTN"
    np.testing.assert_array_equal(_native.pack_queries(b"ACGTN"), one)
    many = _native.pack_queries(["ACG", b"TTT", "NRY"])
    assert many.shape == (3, 3) and many.tobytes() == b"ACGTTTNRY"
    np.testing.assert_array_equal(_native.pack_queries(("ACG", "TTT", "NRY")), many)
    arr = np.frombuffer(b"ACGTTTNRY", dtype=np.uint8).reshape(3, 3)
    np.testing.assert_array_equal(_native.pack_queries(arr), many)
    np.testing.assert_array_equal(_native.pack_queries(arr[:, ::-1])[:, ::-1], many)  # non-contiguous input
    np.testing.assert_array_equal(_native.pack_queries(many, kmer_len=3), many)
    assert _native.pack_queries(["ACG"], kmer_len=3).shape == (1, 3)
    # every letter of the sba alphabet without '$'
    assert _native.pack_queries("ABCDGHKMNRSTVWY").shape == (1, 15)
    # empty batches keep two dimensions
    assert _native.pack_queries([]).shape[0] == 0 and _native.pack_queries([]).ndim == 2
    assert _native.pack_queries([], kmer_len=7).shape == (0, 7)
    assert _native.pack_queries(np.zeros((0, 31), dtype=np.uint8)).shape == (0, 31)


def test_pack_queries_errors():
    with pytest.raises(ValueError, match="differ in length.*k-mer 2"):
        _native.pack_queries(["ACG", "TTT", "AC"])
    with pytest.raises(ValueError, match="k-mer 1 is empty"):
        _native.pack_queries(["ACG", ""])
    with pytest.raises(ValueError, match="empty"):
        _native.pack_queries("")
    with pytest.raises(ValueError, match="empty"):
        _native.pack_queries(np.zeros((3, 0), dtype=np.uint8))
    with pytest.raises(ValueError, match="k-mer 1 holds the character 'a'"):
        _native.pack_queries(["ACG", "TaT"])
    with pytest.raises(ValueError, match=r"k-mer 0 holds the character '\$'"):
        _native.pack_queries("AC$")
    with pytest.raises(ValueError, match="k-mer 2 holds the character 'X'"):
        _native.pack_queries(np.frombuffer(b"ACGTTTAXA", dtype=np.uint8).reshape(3, 3))
    with pytest.raises(ValueError, match="k-mer 0 holds the character"):
        _native.pack_queries("ACé")
    with pytest.raises(ValueError, match="kmer_len is 4"):
        _native.pack_queries(["ACG", "TTT"], kmer_len=4)
    with pytest.raises(ValueError, match="2-D uint8"):
        _native.pack_queries(np.zeros(5, dtype=np.uint8))
    with pytest.raises(ValueError, match="2-D uint8"):
        _native.pack_queries(np.zeros((2, 2), dtype=np.int32))
    with pytest.raises(ValueError, match="neither str nor bytes"):
        _native.pack_queries([5])


def test_lookup_is_exported():
    lib = _native.load_library()
    for name in ("gk_lookup", "gk_copy_strand_range"):
        assert name in _native.EXPORTED and name in _native._SIGS
        assert hasattr(lib, name)
    assert f"int gk_lookup(gk_ctx *ctx, const uint8_t *queries, uint64_t m, uint32_t qlen, uint64_t *first, " \
           f"uint32_t *count);" in (ROOT / "include" / "gkm.h").read_text()


def test_lookup_knobs_are_in_the_table():
    lib = _native.load_library()
    for name, value in (("GKM_LOOKUP_PATH", "bytes"), ("GKM_LOOKUP_PATH", "keys"), ("GKM_LOOKUP_CHUNK", "1500"),
                        ("GKM_LOOKUP_DIR", "0")):
        _native.options[name] = value
        assert _native.options.get(name) == value
        del _native.options[name]
        assert name not in _native.options
    for name in (b"GKM_LOOKUP_PATHS", b"GKM_LOOKUP", b"GKM_LOOKUP_CHUNKS", b"GKM_LOOKUP_DIRS", b"gkm_lookup_path"):
        assert lib.gk_set_option(name, b"1") == _native.GK_E_ARG
    # the lookup knobs are not operational ones: the environment does not set them (gk_set_option only)
    text = (ROOT / "genome-kmers_amd" / "csrc" / "gkm_capi.hip").read_text()
    for name in ("GKM_LOOKUP_PATH", "GKM_LOOKUP_CHUNK", "GKM_LOOKUP_DIR"):
        assert f'{{"{name}", false}}' in text


def test_null_context_and_empty_batch():
    lib = _native.load_library()
    assert lib.gk_lookup(None, None, 0, 5, None, None) == _native.GK_E_ARG
    assert lib.gk_lookup(None, None, 3, 5, None, None) == _native.GK_E_ARG


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
    exe = tmp_path / "lookup_asan"
    r = subprocess.run(["g++", *SAN_FLAGS, "-I", str(ROOT / "genome-kmers_amd" / "csrc"),
                        str(ROOT / "tests" / "sanitize" / "lookup_driver.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    bad = ("AddressSanitizer", "runtime error:", "LeakSanitizer")
    assert r.returncode == 0 and not any(b in r.stderr for b in bad), (r.returncode, r.stderr[-3000:])
    assert r.stdout.strip() == "ok"
