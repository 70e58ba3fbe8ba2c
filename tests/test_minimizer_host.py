"""gk_minimizers / Kmers.minimizers, the parts that need no GPU: the exported symbols and their
declarations, the chunk knob of gk_set_option, the Python layer's argument checks, and the host-only C++
(order hash, canonical key, the local rule, the two-sided chunk arithmetic:
genome-kmers_amd/csrc/gkm_minimizer_host.h) under ``-fsanitize=address,undefined`` in a stand-alone
driver (tests/sanitize/minimizer_driver.cpp) that is handed tests/minimizerref.py's answers in a file."""

import os
import shutil
import subprocess

import numpy as np
import pytest

import minimizerref as ref
from conftest import ROOT
from genome_kmers import _native
from genome_kmers.kmers import Kmers, MinimizerResult

SYMBOLS = ("gk_minimizers", "gk_copy_minimizers", "gk_device_minimizers", "gk_select_minimizers")


def test_symbols_are_exported_and_declared():
    lib = _native.load_library()
    header = (ROOT / "include" / "gkm.h").read_text()
    for name in SYMBOLS:
        assert name in _native.EXPORTED and name in _native._SIGS and hasattr(lib, name)
    assert "#define GK_MINIMIZER_CANONICAL 1u" in header and "#define GK_MINIMIZER_LEX       2u" in header
    assert ("int gk_minimizers(gk_ctx *ctx, const uint8_t *seqs, const uint64_t *offsets, uint64_t nseq,\n"
            "                  uint32_t k, uint32_t w, uint32_t flags, uint64_t *n_out, uint32_t *per_seq);") in header
    assert "int gk_copy_minimizers(gk_ctx *ctx, uint64_t *pos, uint64_t *key, uint8_t *strand, uint64_t n);" in header
    assert "int gk_device_minimizers(gk_ctx *ctx, void **pos, void **key, void **strand, uint64_t *n);" in header
    assert "int gk_select_minimizers(gk_ctx *ctx, uint32_t k, uint32_t w, uint32_t flags, uint64_t *n_out);" in header
    assert _native.MINIMIZER_CANONICAL == 1 and _native.MINIMIZER_LEX == 2
    assert len(_native._SIGS["gk_minimizers"][0]) == 9 and len(_native._SIGS["gk_copy_minimizers"][0]) == 5
    assert len(_native._SIGS["gk_device_minimizers"][0]) == 5 and len(_native._SIGS["gk_select_minimizers"][0]) == 5
    assert MinimizerResult._fields == ("offsets", "pos", "keys", "strands")
    text = (ROOT / "genome-kmers_amd" / "csrc" / "Makefile").read_text()
    assert "gkm_minimizer.hip" in text


def test_null_context():
    lib = _native.load_library()
    assert lib.gk_minimizers(None, None, None, 0, 15, 10, 0, None, None) == _native.GK_E_ARG
    assert lib.gk_copy_minimizers(None, None, None, None, 0) == _native.GK_E_ARG
    assert lib.gk_device_minimizers(None, None, None, None, None) == _native.GK_E_ARG
    assert lib.gk_select_minimizers(None, 15, 10, 0, None) == _native.GK_E_ARG


def test_chunk_knob_is_in_the_table():
    lib = _native.load_library()
    _native.options["GKM_MINIMIZER_CHUNK"] = "1500"
    assert _native.options.get("GKM_MINIMIZER_CHUNK") == "1500"
    del _native.options["GKM_MINIMIZER_CHUNK"]
    assert "GKM_MINIMIZER_CHUNK" not in _native.options
    for name in (b"GKM_MINIMIZER_CHUNKS", b"GKM_MINIMIZER", b"GKM_MINIMIZER_PATH", b"gkm_minimizer_chunk"):
        assert lib.gk_set_option(name, b"1") == _native.GK_E_ARG
    # not an operational knob: the environment does not set it (gk_set_option only)
    text = (ROOT / "genome-kmers_amd" / "csrc" / "gkm_capi.hip").read_text()
    assert '{"GKM_MINIMIZER_CHUNK", false}' in text


def test_python_layer_checks_need_no_device():
    km = Kmers(min_kmer_len=15, max_kmer_len=15)
    for kwargs, match in (({"w": 0}, "w must be in 1..256"), ({"w": 257}, "w must be in 1..256"),
                          ({"w": 10, "kmer_len": 33}, "must be in 1..32"), ({"w": 10, "kmer_len": 0}, "must be in 1..32"),
                          ({"w": 10, "order": "random"}, "order must be 'hash' or 'lex'")):
        with pytest.raises(ValueError, match=match):
            km.minimizers("ACGTACGTACGTACGTACGT", **kwargs)
    with pytest.raises(ValueError, match="needs kmer_len"):
        Kmers(min_kmer_len=15).minimizers("ACGT", 4)
    with pytest.raises(ValueError, match="outside the alphabet"):
        km.minimizers("ACGTacgt", 4)
    for lo, hi in ((15, None), (15, 16), (33, 33)):
        with pytest.raises(ValueError, match="select_minimizers needs min_kmer_len == max_kmer_len <= 32"):
            Kmers(min_kmer_len=lo, max_kmer_len=hi).select_minimizers(10)
    with pytest.raises(ValueError, match="w must be in 1..256"):
        km.select_minimizers(300)
    with pytest.raises(ValueError, match="order must be"):
        km.select_minimizers(10, order="stable")
    with pytest.raises(ValueError, match="chosen by select_minimizers"):
        km.find_minimizers("ACGTACGTACGTACGTACGT")


SAN_FLAGS = ["-std=c++17", "-g", "-O1", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=all"]


def write_cases(path):
    rng = np.random.default_rng(23)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)

    def rnd(n):
        return bytes(rng.choice(acgt, n))

    holes = bytearray(rnd(700))
    for p in (0, 90, 91, 300, 512, 699):
        holes[p] = ord("N")
    holes[400] = ord("$")
    batches = [
        [rnd(900)],
        [b"A" * 400 + rnd(50) + b"T" * 300],
        [b"AC" * 200, b"ACG" * 150],
        [bytes(holes)],
        [rnd(n) for n in (120, 0, 31, 32, 1, 0, 0, 200, 7, 64, 0)],
        [b"", b""],
    ]
    params = [(1, 1, 0), (1, 4, 2), (2, 3, 1), (3, 10, 0), (15, 10, 1), (16, 19, 3), (31, 64, 0), (32, 2, 1),
              (32, 256, 2), (5, 256, 0)]
    lines, n = [], 0
    for seqs in batches:
        arr, off = ref.as_batch(seqs)
        for k, w, flags in params:
            pos, key, strand, _ = ref.by_windows(arr, off, k, w, canonical=bool(flags & 1), lex=bool(flags & 2))
            lines.append(f"{k} {w} {flags} {off.size - 1} {pos.size}")
            lines.append(" ".join(map(str, off.tolist())))
            lines.append(arr.tobytes().decode() or "-")
            for a in (pos, key, strand):
                lines.append(" ".join(map(str, a.tolist())))
            n += 1
    path.write_text(f"{n}\n" + "\n".join(lines) + "\n")
    return n


def test_host_pieces_under_asan_ubsan(tmp_path):
    # the only thing that may skip: no g++, or a g++ without the sanitizer runtime, shown by a
    # one-line program that does not build with the same flags
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if shutil.which("g++") is None or subprocess.run(
            ["g++", *SAN_FLAGS, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("no g++ with the address / undefined-behaviour sanitizer runtime")
    exe = tmp_path / "minimizer_asan"
    r = subprocess.run(["g++", *SAN_FLAGS, "-I", str(ROOT / "genome-kmers_amd" / "csrc"),
                        str(ROOT / "tests" / "sanitize" / "minimizer_driver.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    cases = tmp_path / "cases.txt"
    assert write_cases(cases) == 60
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe), str(cases)], capture_output=True, text=True, env=env, timeout=300)
    bad = ("AddressSanitizer", "runtime error:", "LeakSanitizer")
    assert r.returncode == 0 and not any(b in r.stderr for b in bad), (r.returncode, r.stderr[-3000:])
    assert r.stdout.strip() == "ok"
