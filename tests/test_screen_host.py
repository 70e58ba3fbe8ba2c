"""gk_screen / Kmers.screen, the parts that need no GPU: read packing (_native.pack_sequences), the
exported symbol and its declaration, the screen knobs of gk_set_option, and the host-only C++ (offset
validation, chunk and overlap arithmetic, position to sequence, the knobs' values:
genome-kmers_amd/csrc/gkm_screen_host.h) under ``-fsanitize=address,undefined`` in a stand-alone driver
(tests/sanitize/screen_driver.cpp)."""

import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from genome_kmers import _native


def test_pack_sequences_input_forms():
    arr, off = _native.pack_sequences("ACGTN")
    assert arr.dtype == np.uint8 and off.dtype == np.uint64 and arr.flags.c_contiguous
    assert arr.tobytes() == b"ACGTN" and off.tolist() == [0, 5]
    arr2, off2 = _native.pack_sequences(b"ACGTN")
    assert arr2.tobytes() == b"ACGTN" and off2.tolist() == [0, 5]
    arr, off = _native.pack_sequences(["ACG", b"", "T", bytearray(b"NRYACGT"), ""])
    assert arr.tobytes() == b"ACGTNRYACGT" and off.tolist() == [0, 3, 3, 4, 11, 11]
    arr3, off3 = _native.pack_sequences(("ACG", "", "T", "NRYACGT", ""))  # a tuple of reads is a list of reads
    assert arr3.tobytes() == arr.tobytes() and off3.tolist() == off.tolist()
    # an already packed pair passes through (offsets of any integer type)
    for dtype in (np.uint64, np.int64, np.int32, np.uint32):
        arr4, off4 = _native.pack_sequences((arr, off.astype(dtype)))
        assert arr4.tobytes() == arr.tobytes() and off4.dtype == np.uint64 and off4.tolist() == off.tolist()
    big = np.frombuffer(b"AACCGGTT", dtype=np.uint8)
    arr5, _ = _native.pack_sequences((big[::2], np.array([0, 2, 4])))  # non-contiguous input
    assert arr5.flags.c_contiguous and arr5.tobytes() == b"ACGT"
    # every letter of the sba alphabet without '$'
    assert _native.pack_sequences("ABCDGHKMNRSTVWY")[0].size == 15
    # empty batches and batches of empty reads
    arr, off = _native.pack_sequences([])
    assert arr.size == 0 and arr.dtype == np.uint8 and off.tolist() == [0]
    arr, off = _native.pack_sequences(["", "", ""])
    assert arr.size == 0 and off.tolist() == [0, 0, 0, 0]
    arr, off = _native.pack_sequences("")
    assert arr.size == 0 and off.tolist() == [0, 0]


def test_pack_sequences_errors():
    with pytest.raises(ValueError, match="sequence 1 holds the character 'a' at offset 1"):
        _native.pack_sequences(["ACG", "TaT"])
    with pytest.raises(ValueError, match=r"sequence 0 holds the character '\$' at offset 2"):
        _native.pack_sequences("AC$")
    with pytest.raises(ValueError, match="sequence 3 holds the character 'X' at offset 0"):
        _native.pack_sequences(["ACG", "", "", "XA"])
    with pytest.raises(ValueError, match="sequence 1 holds the character 'é' at offset 2"):
        _native.pack_sequences(["A", "ACé"])
    packed = (np.frombuffer(b"ACGTTTAXA", dtype=np.uint8), np.array([0, 3, 3, 9], dtype=np.uint64))
    with pytest.raises(ValueError, match="sequence 2 holds the character 'X' at offset 4"):
        _native.pack_sequences(packed)
    with pytest.raises(ValueError, match="neither str nor bytes"):
        _native.pack_sequences(["ACG", 5])
    arr = np.frombuffer(b"ACGTACGT", dtype=np.uint8)
    for offsets in ([1, 8], [0, 5, 4, 8], [0, 7], [0, 9], []):
        with pytest.raises(ValueError, match="offsets must"):
            _native.pack_sequences((arr, np.array(offsets, dtype=np.uint64)))
    with pytest.raises(ValueError, match="offsets must"):
        _native.pack_sequences((arr, np.array([0, -1, 8], dtype=np.int64)))
    with pytest.raises(ValueError, match="offsets must"):
        _native.pack_sequences((arr, np.array([0.0, 8.0])))
    with pytest.raises(ValueError, match="1-D uint8"):
        _native.pack_sequences((arr.reshape(2, 4), np.array([0, 8])))
    with pytest.raises(ValueError, match="1-D uint8"):
        _native.pack_sequences((arr.astype(np.int32), np.array([0, 8])))


def test_screen_is_exported():
    lib = _native.load_library()
    assert "gk_screen" in _native.EXPORTED and "gk_screen" in _native._SIGS
    assert hasattr(lib, "gk_screen")
    header = (ROOT / "include" / "gkm.h").read_text()
    assert "#define GK_SCREEN_BOTH_STRANDS 1u" in header
    assert ("int gk_screen(gk_ctx *ctx, const uint8_t *seqs, const uint64_t *offsets, uint64_t nseq, uint32_t flags,\n"
            "              uint32_t *n_present, uint64_t *occurrences, uint32_t *window_count);") in header
    assert _native.SCREEN_BOTH_STRANDS == 1


def test_screen_knobs_are_in_the_table():
    lib = _native.load_library()
    for name, value in (("GKM_SCREEN_PATH", "bytes"), ("GKM_SCREEN_PATH", "keys"), ("GKM_SCREEN_CHUNK", "1500")):
        _native.options[name] = value
        assert _native.options.get(name) == value
        del _native.options[name]
        assert name not in _native.options
    for name in (b"GKM_SCREEN_PATHS", b"GKM_SCREEN", b"GKM_SCREEN_CHUNKS", b"GKM_SCREEN_DIR", b"gkm_screen_path"):
        assert lib.gk_set_option(name, b"1") == _native.GK_E_ARG
    # the screen knobs are not operational ones: the environment does not set them (gk_set_option only)
    text = (ROOT / "genome-kmers_amd" / "csrc" / "gkm_capi.hip").read_text()
    for name in ("GKM_SCREEN_PATH", "GKM_SCREEN_CHUNK"):
        assert f'{{"{name}", false}}' in text
    # (the values a call refuses -- a path other than bytes / keys -- and the chunk values that fall
    # back to the default are parse_path / chunk_bytes, checked by the driver below)


def test_null_context_and_empty_batch():
    lib = _native.load_library()
    assert lib.gk_screen(None, None, None, 0, 0, None, None, None) == _native.GK_E_ARG
    assert lib.gk_screen(None, None, None, 3, 0, None, None, None) == _native.GK_E_ARG


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
    exe = tmp_path / "screen_asan"
    r = subprocess.run(["g++", *SAN_FLAGS, "-I", str(ROOT / "genome-kmers_amd" / "csrc"),
                        str(ROOT / "tests" / "sanitize" / "screen_driver.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    bad = ("AddressSanitizer", "runtime error:", "LeakSanitizer")
    assert r.returncode == 0 and not any(b in r.stderr for b in bad), (r.returncode, r.stderr[-3000:])
    assert r.stdout.strip() == "ok"
