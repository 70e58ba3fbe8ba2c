"""gk_match / Kmers.match_lengths, maximal_matches: the parts that need no GPU -- the exported symbol
and its declaration, the match knobs of gk_set_option, the null-context and Python argument checks (made
before any device call), and the plain C++ of genome-kmers_amd/csrc/gkm_match_host.h (the neighbour
comparison of both paths, the byte path's per-position routine, the packed maximum, the chunk
arithmetic at an overlap of C - 1) under ``-fsanitize=address,undefined`` in a stand-alone driver
(tests/sanitize/match_driver.cpp) whose answers must equal tests/matchref.py's.  Nothing is loaded into
Python under a sanitizer."""

import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import matchref
from conftest import ROOT
from genome_kmers import _native
from genome_kmers import kmers as gk
from genome_kmers.kmers import MatchResult, maximal_from_lengths  # noqa: F401  (the feature under test)


def test_match_is_exported():
    lib = _native.load_library()
    assert "gk_match" in _native.EXPORTED and "gk_match" in _native._SIGS
    assert hasattr(lib, "gk_match")
    header = (ROOT / "include" / "gkm.h").read_text()
    assert ("int gk_match(gk_ctx *ctx, const uint8_t *seqs, const uint64_t *offsets, uint64_t nseq, uint32_t max_len,\n"
            "             uint32_t flags, uint32_t *longest, uint32_t *longest_pos, uint64_t *sum_len,\n"
            "             uint32_t *match_len, uint64_t *match_first, uint32_t *match_count);") in header
    assert callable(_native.Engine.match)
    for method in ("match_lengths", "maximal_matches"):
        assert callable(getattr(gk.Kmers, method))
    assert MatchResult._fields == ("longest", "longest_pos", "sum_len", "lengths", "first", "count", "offsets")
    assert gk.MAX_MATCH_LEN == 4096


def test_constants_the_gpu_tests_mirror():
    """tests/test_gpu_match.py places its edges by these values."""
    text = (ROOT / "genome-kmers_amd" / "csrc" / "gkm_match.hip").read_text()
    values = {name: int(v) for name, v in re.findall(r"constexpr int (k\w+) = (\d+);", text)}
    assert (values["kMatchThreads"], values["kMatchBounds"], values["kMatchHalo"]) == (256, 256, 31)
    assert "#define GKM_MATCH_WIN 4\n" in text
    host = (ROOT / "genome-kmers_amd" / "csrc" / "gkm_match_host.h").read_text()
    assert "constexpr uint32_t kMaxCap = 4096;" in host and "constexpr uint64_t kChunkBytes = 4ull << 20;" in host


def test_match_knobs_are_in_the_table():
    lib = _native.load_library()
    for name, value in (("GKM_MATCH_PATH", "bytes"), ("GKM_MATCH_PATH", "keys"), ("GKM_MATCH_CHUNK", "1500")):
        _native.options[name] = value
        assert _native.options.get(name) == value
        del _native.options[name]
        assert name not in _native.options
    for name in (b"GKM_MATCH_PATHS", b"GKM_MATCH", b"GKM_MATCH_CHUNKS", b"GKM_MATCH_DIR", b"gkm_match_path"):
        assert lib.gk_set_option(name, b"1") == _native.GK_E_ARG
    # not operational knobs: the environment does not set them (gk_set_option only)
    text = (ROOT / "genome-kmers_amd" / "csrc" / "gkm_capi.hip").read_text()
    for name in ("GKM_MATCH_PATH", "GKM_MATCH_CHUNK"):
        assert f'{{"{name}", false}}' in text


def test_null_context_and_empty_batch():
    lib = _native.load_library()
    assert lib.gk_match(None, None, None, 0, 0, 0, None, None, None, None, None, None) == _native.GK_E_ARG
    assert lib.gk_match(None, None, None, 3, 31, 0, None, None, None, None, None, None) == _native.GK_E_ARG


def host_kmers(kmin, kmax, is_sorted=True):
    """A Kmers with no sequence collection and no engine: the state the argument checks read."""
    km = gk.Kmers(None, min_kmer_len=kmin, max_kmer_len=kmax)
    km._is_sorted = is_sorted
    return km


@pytest.mark.parametrize("method", ["match_lengths", "maximal_matches"])
def test_python_argument_checks_need_no_device(method):
    def call(km, *args, **kw):
        if method == "maximal_matches":
            return km.maximal_matches("ACGT", 2, *args, **kw)
        return km.match_lengths("ACGT", *args, **kw)

    with pytest.raises(AssertionError, match="must be sorted when calling match_lengths"):
        call(host_kmers(21, 21, is_sorted=False))
    km = host_kmers(8, 21)
    for bad in (0, -3):
        with pytest.raises(ValueError, match=rf"max_len \({bad}\) must be >= 1"):
            call(km, bad)
    for bad in (2.0, "7", True, [3]):
        with pytest.raises(ValueError, match="max_len must be an int >= 1"):
            call(km, bad)
    with pytest.raises(ValueError, match=r"max_len \(22\) is greater than max_kmer_len \(21\)"):
        call(km, 22)
    with pytest.raises(ValueError, match=r"max_len \(22\) is greater than max_kmer_len \(21\)"):
        call(km, np.int64(22))
    other = host_kmers(21, 21)
    other.kmer_source_strand = "both"
    with pytest.raises(ValueError, match="kmer_source_strand 'forward' \\('both'\\)"):
        call(other, 5)
    canon = host_kmers(21, 21)
    canon._canonical = True
    with pytest.raises(ValueError, match="match_lengths needs a forward order: canonical k-mers have no prefixes"):
        call(canon)
    suffix = host_kmers(5, None)
    with pytest.raises(ValueError, match="match_lengths needs max_len when max_kmer_len is None"):
        call(suffix)
    with pytest.raises(ValueError, match=r"max_len \(4097\) is greater than 4096"):
        call(suffix, 4097)
    if method == "maximal_matches":
        for bad in (0, -1, 2.5, True):
            with pytest.raises(ValueError, match="min_len must be an int >= 1"):
                km.maximal_matches("ACGT", bad)


# ---------------------------------------------------------------------------------------------
# the plain C++ under the host sanitizers
# ---------------------------------------------------------------------------------------------
SAN_FLAGS = ["-std=c++17", "-g", "-O1", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=all"]
SAN_ENV = dict(ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    # the only thing that may skip: no g++, or a g++ without the sanitizer runtime, shown by a
    # one-line program that does not build with the same flags
    tmp = tmp_path_factory.mktemp("match_asan")
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if shutil.which("g++") is None or subprocess.run(
            ["g++", *SAN_FLAGS, str(probe), "-o", str(tmp / "probe")], capture_output=True).returncode != 0:
        pytest.skip("no g++ with the address / undefined-behaviour sanitizer runtime")
    exe = tmp / "match_asan"
    r = subprocess.run(["g++", *SAN_FLAGS, "-I", str(ROOT / "genome-kmers_amd" / "csrc"),
                        str(ROOT / "tests" / "sanitize" / "match_driver.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_driver(exe, *args):
    r = subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True, env=dict(os.environ, **SAN_ENV),
                       timeout=120)
    bad = ("AddressSanitizer", "runtime error:", "LeakSanitizer")
    assert r.returncode == 0 and not any(b in r.stderr for b in bad), (r.returncode, r.stderr[-3000:])
    return r.stdout


def test_edge_cases_under_asan_ubsan(driver):
    assert run_driver(driver, "self").strip() == "ok"


def rand_seq(seed, n, letters="ACGT") -> str:
    rng = np.random.default_rng(seed)
    return np.frombuffer(letters.encode(), dtype=np.uint8)[rng.integers(0, len(letters), n)].tobytes().decode()


def host_genome(letters):
    a = rand_seq(41, 700, letters)
    # contigs of every length 1..12: a '$' on the index side at every offset of a short match
    tails = [(f"t{i}", a[100:100 + i]) for i in range(1, 13)]
    return [("c0", a), ("c1", a[200:300] + rand_seq(42, 150, letters)), ("polyA", "A" * 60), ("polyT", "T" * 40)] + tails + \
           [("last", rand_seq(43, 30, letters) + a[100:109])]   # the sba ends inside a repeat: its last byte is read


def host_reads(genome, with_n):
    a = genome[0][1]
    reads = [a[50:200], "", a[95:125], rand_seq(44, 120), "T" * 45, "A" * 70, a[100:112] + "G", a[690:700] + a[:30], "C",
             genome[-1][1][-9:] + "A", genome[-1][1][-5:], a[100:109]]
    if with_n:
        reads += [a[300:320] + "N" + a[321:350], "NN", "N" + a[5:40]]
    return reads


def parse(out, total):
    rows = np.array([line.split() for line in out.splitlines()], dtype=np.int64).reshape(-1, 3)
    assert rows.shape[0] == total
    return rows[:, 0], rows[:, 1], rows[:, 2]


def assert_rows(out, ref, note):
    lengths, first, count = parse(out, len(ref["lengths"]))
    np.testing.assert_array_equal(lengths, ref["lengths"].astype(np.int64), err_msg=f"{note} lengths")
    np.testing.assert_array_equal(first, ref["first"].astype(np.int64), err_msg=f"{note} first")
    np.testing.assert_array_equal(count, ref["count"].astype(np.int64), err_msg=f"{note} count")


@pytest.mark.parametrize("letters,min_len,max_len,cap", [
    ("ACGT", 12, 12, 12), ("ACGT", 31, 31, 31), ("ACGT", 40, 40, 40), ("ACGT", 3, 3, 3), ("ACGT", 31, 31, 7),
    ("ACGT", 1, 12, 12), ("ACGT", 5, 24, 24), ("ACGT", 1, None, 12), ("ACGT", 1, None, 40), ("ACGTN", 1, None, 25),
    ("ACGTNRY", 6, 16, 16),
])
def test_byte_path_equals_the_reference(driver, tmp_path, letters, min_len, max_len, cap):
    genome = host_genome(letters)
    reads = host_reads(genome, with_n=True)
    sba = matchref.as_sba(genome)
    index = matchref.Index(sba, min_len, max_len, cap)
    ref = matchref.match(index, reads)
    v = ref["lengths"]
    assert (v == cap).any() and ((v > 0) & (v < cap)).any() and (ref["count"] > 1).any()
    assert (v == 0).any() or letters != "ACGT"  # (an N of a read matches an N of the genome)
    if min_len < cap:
        assert (index.lens < cap).any()  # k-mers that a '$' (or the sba's end) cuts short are in the index
    order = np.argsort(index.rows.view(f"S{cap}").ravel(), kind="stable")
    starts = index.starts[order].astype(np.uint32)
    arr, offsets = matchref.pack(reads)
    path = tmp_path / "case.bin"
    path.write_bytes(np.array([len(sba), len(starts), len(arr), len(offsets) - 1, cap], dtype=np.uint64).tobytes()
                     + sba.tobytes() + starts.tobytes() + arr.tobytes() + offsets.astype(np.uint64).tobytes())
    assert_rows(run_driver(driver, "bytes", path), ref, f"bytes {letters} {min_len} {max_len} {cap}")


def encode2(rows):
    """uint64 keys of [n, K] A/C/G/T rows: 2 bits per symbol (A0 C1 G2 T3), the first symbol on top"""
    code = np.zeros(256, dtype=np.uint64)
    for i, ch in enumerate(b"ACGT"):
        code[ch] = i
    keys = np.zeros(rows.shape[0], dtype=np.uint64)
    for t in range(rows.shape[1]):
        keys = (keys << np.uint64(2)) | code[rows[:, t]]
    return keys


@pytest.mark.parametrize("K,cap", [(1, 1), (3, 3), (12, 12), (12, 5), (31, 31), (32, 32), (32, 9)])
def test_key_path_equals_the_reference(driver, tmp_path, K, cap):
    genome = host_genome("ACGT")
    reads = host_reads(genome, with_n=True) + ["T" * 33 + "A" * 33 + "T"]
    sba = matchref.as_sba(genome)
    index = matchref.Index(sba, K, K, cap)
    ref = matchref.match(index, reads)
    v = ref["lengths"]
    assert (v == cap).any() and (v == 0).any() and (ref["count"] > 1).any()
    full = matchref.Index(sba, K, K, K)
    keys = np.sort(encode2(full.rows))
    if K == 32:  # the words 0 (all A) and 2^64 - 1 (all T) are keys
        assert keys[0] == 0 and keys[-1] == np.uint64(0xFFFFFFFFFFFFFFFF)
    arr, offsets = matchref.pack(reads)
    path = tmp_path / "case.bin"
    path.write_bytes(np.array([K, len(keys), len(arr), len(offsets) - 1, cap], dtype=np.uint64).tobytes()
                     + keys.tobytes() + arr.tobytes() + offsets.astype(np.uint64).tobytes())
    assert_rows(run_driver(driver, "keys", path), ref, f"keys {K} {cap}")
